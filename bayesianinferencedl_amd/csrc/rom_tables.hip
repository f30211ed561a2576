// Host-only tables of the reduced model: the descriptor validators, the pattern-uniform k-steps and their packers, the grouped
// tables, the half lists of a mirror-symmetric ROM.  No kernel and no HIP runtime call (rom_tables.h: what api_rom.hip uses).
#include "rom_tables.h"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <iterator>
#include <map>

namespace finrom {

int validate_rom_desc(const finrom_rom_desc* a) {
  if (a->n <= 0 || a->r <= 0 || a->P < 0 || a->P > 31 || a->n_obs < 0 || a->nterms < 0) { set_error("rom_create: inconsistent sizes"); return FINROM_ERR_ARG; }
  if (!a->row_ptr || (a->nterms > 0 && (!a->term_p || !a->term_val))) { set_error("rom_create: null table"); return FINROM_ERR_ARG; }
  if (a->row_ptr[0] != 0 || a->row_ptr[a->n] != a->nterms) { set_error("rom_create: invalid row_ptr"); return FINROM_ERR_ARG; }
  for (int i = 0; i < a->n; ++i) if (a->row_ptr[i + 1] < a->row_ptr[i]) { set_error("rom_create: invalid row_ptr"); return FINROM_ERR_ARG; }
  for (int t = 0; t < a->nterms; ++t) if (a->term_p[t] < 0 || a->term_p[t] > a->P) { set_error("rom_create: invalid term_p"); return FINROM_ERR_ARG; }
  // a row lists each theta index at most once: the pattern-uniform k-step tables below fill a slot with the SUM of the row's
  // terms that carry the slot's index, so a repeated index would be counted once per repetition
  for (int i = 0; i < a->n; ++i) {
    unsigned seen = 0;
    for (int t = a->row_ptr[i]; t < a->row_ptr[i + 1]; ++t) {
      if (seen & (1u << a->term_p[t])) { set_error("rom_create: a row of psi lists the same theta index twice (merge the terms)"); return FINROM_ERR_ARG; }
      seen |= 1u << a->term_p[t];
    }
  }
  return 0;
}

int validate_row_weights(const finrom_rom_desc* a, const double* row_weight) {
  for (int i = 0; i < a->n; ++i)
    if (row_weight[i] != 1.0 && row_weight[i] != 2.0) { set_error("rom_mirror: a row weight is neither 1 nor 2"); return FINROM_ERR_ARG; }
  return 0;
}

// rows with a term, sorted by term count (descending)
std::vector<int> rows_by_term_count(const finrom_rom_desc* a) {
  auto cnt = [&](int row) { return a->row_ptr[row + 1] - a->row_ptr[row]; };
  std::vector<int> order;
  for (int i = 0; i < a->n; ++i) if (cnt(i) > 0) order.push_back(i);
  std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return cnt(x) > cnt(y); });
  return order;
}

namespace {      // the packers: nothing outside this file calls them
constexpr int kMaxTerms = 4;      // terms per row of a k-step (rom_proj_device.h: the loops' slot count)
// multiplies / multiply-adds per block that proj_main_grouped's `finish` spends on a k-step of this pattern (build_grouped_tables)
// (group0: the k-step sits in segment 0 with its usual coefficients -- a lone theta_d then multiplies its rows)
int kstep_vector_ops(const std::vector<int>& pat, bool group0 = false) {
  const int nt = (int)pat.size();
  if (nt == 1) return group0 && pat[0] != 0 ? 1 : 0;                             // T_d or T_0 as loaded
  if (nt == 2 && (pat[0] == 0) != (pat[1] == 0)) return 1;                       // group d: T_d + (1 / theta_d) T_0
  return nt - (std::find(pat.begin(), pat.end(), 0) == pat.begin() ? 1 : 0);     // group 0: the first coefficient is 1 only for T_0
}
// When a leading parameter is worth a group (build_grouped_tables, scale_free).  The grouped form pays for itself on the k-steps
// whose pattern is {theta_d} ALONE: divided by theta_d their rows are the slab as loaded, NB multiplies saved each.  A k-step
// {1, theta_d} costs NB multiply-adds either way, T_d + (1 / theta_d) T_0 in the group or theta_d T_d + T_0 at scale 1.  Every group
// costs a rescale of the accumulators, 4 multiplies on each of the NB (NB + 1) / 2 tiles behind a drain of the matrix pipe (five
// s_nop 15 and a fence: about as long as kRescaleDrainOps multiplies).  So d becomes a group only if
//   NB x (its {theta_d}-alone k-steps)  >  2 NB (NB + 1) + kRescaleDrainOps;
// otherwise its k-steps go to segment 0 with their usual coefficients.  The rule is applied per weight class (a group is a run
// of one class) and only to a descriptor with term-less rows, the short half list (the trigger of PACK_FEWEST): that list has lost
// the interior rows that carry {theta_d} alone.  Every other list is built as it always was.
constexpr int kRescaleDrainOps = 20;
bool group_pays(int alone_ksteps, int NB) { return alone_ksteps * NB > 2 * NB * (NB + 1) + kRescaleDrainOps; }
struct PackCost {
  int ksteps = 0, fma_ksteps = 0, fma = 0;
  bool operator<(const PackCost& o) const { return ksteps != o.ksteps ? ksteps < o.ksteps : fma_ksteps != o.fma_ksteps ? fma_ksteps < o.fma_ksteps : fma < o.fma; }
};
PackCost pack_cost(const std::vector<KStep>& ks) {
  PackCost c;
  for (const KStep& k : ks) { const int ops = kstep_vector_ops(k.pat); ++c.ksteps; c.fma_ksteps += ops > 0; c.fma += ops; }
  return c;
}
typedef std::vector<std::pair<std::vector<int>, std::vector<int>>> LeftClasses;      // (pattern, its 1..3 left-over rows)
std::vector<KStep> pack_consecutive(const LeftClasses& cls) {
  std::vector<KStep> out;
  KStep cur{{}, {-1, -1, -1, -1}};
  int fill = 0;
  auto flush = [&]() { if (fill) out.push_back(cur); cur = KStep{{}, {-1, -1, -1, -1}}; fill = 0; };
  for (const auto& c : cls)
    for (int row : c.second) {
      std::vector<int> u = cur.pat;
      for (int pp : c.first) if (std::find(u.begin(), u.end(), pp) == u.end()) u.push_back(pp);
      if (fill == 4 || (int)u.size() > kMaxTerms) { flush(); u = c.first; }
      cur.pat = u; cur.rows[fill++] = row;
    }
  flush();
  return out;
}
std::vector<KStep> pack_padded(const LeftClasses& cls) {
  std::vector<KStep> out;
  for (const auto& c : cls) {
    KStep k{c.first, {-1, -1, -1, -1}};
    for (size_t i = 0; i < c.second.size() && i < 4; ++i) k.rows[i] = c.second[i];
    out.push_back(k);
  }
  return out;
}
// nested: the classes with the longest patterns open k-steps; a class joins the k-step with room whose pattern CONTAINS its own
// (the shortest such pattern, then the tightest room) -- the k-step then costs what it cost before, the guest's missing terms are
// zero rows -- and is split over several if need be; what stays partly filled is then merged pairwise, smallest union first,
// while the union has at most kMaxTerms entries and the rows fit.
std::vector<KStep> pack_nested(const LeftClasses& cls_in) {
  struct Bin { std::vector<int> pat, rows; };
  LeftClasses cls(cls_in);
  for (auto& c : cls) std::sort(c.first.begin(), c.first.end());
  std::stable_sort(cls.begin(), cls.end(), [](const auto& x, const auto& y) { return x.first.size() > y.first.size(); });
  std::vector<Bin> bins;
  for (const auto& c : cls) {
    size_t next = 0;
    while (next < c.second.size()) {
      const int pending = (int)(c.second.size() - next);
      int best = -1;
      for (int b = 0; b < (int)bins.size(); ++b) {
        const int room = 4 - (int)bins[b].rows.size();
        if (room <= 0 || !std::includes(bins[b].pat.begin(), bins[b].pat.end(), c.first.begin(), c.first.end())) continue;
        if (best < 0) { best = b; continue; }
        const int broom = 4 - (int)bins[best].rows.size();
        if (bins[b].pat.size() != bins[best].pat.size()) { if (bins[b].pat.size() < bins[best].pat.size()) best = b; continue; }
        const bool fits = room >= pending, bfits = broom >= pending;
        if (fits != bfits ? fits : (fits ? room < broom : room > broom)) best = b;
      }
      if (best < 0) { bins.push_back({c.first, {}}); best = (int)bins.size() - 1; }
      while (next < c.second.size() && bins[best].rows.size() < 4) bins[best].rows.push_back(c.second[next++]);
    }
  }
  for (;;) {
    int bi = -1, bj = -1; size_t bu = 0;
    for (int i = 0; i < (int)bins.size(); ++i)
      for (int j = i + 1; j < (int)bins.size(); ++j) {
        if (bins[i].rows.size() + bins[j].rows.size() > 4) continue;
        std::vector<int> u;
        std::set_union(bins[i].pat.begin(), bins[i].pat.end(), bins[j].pat.begin(), bins[j].pat.end(), std::back_inserter(u));
        if ((int)u.size() > kMaxTerms) continue;
        if (bi < 0 || u.size() < bu) { bi = i; bj = j; bu = u.size(); }
      }
    if (bi < 0) break;
    std::vector<int> u;
    std::set_union(bins[bi].pat.begin(), bins[bi].pat.end(), bins[bj].pat.begin(), bins[bj].pat.end(), std::back_inserter(u));
    bins[bi].pat = u;
    bins[bi].rows.insert(bins[bi].rows.end(), bins[bj].rows.begin(), bins[bj].rows.end());
    bins.erase(bins.begin() + bj);
  }
  std::vector<KStep> out;
  for (const Bin& b : bins) {
    KStep k{b.pat, {-1, -1, -1, -1}};
    for (size_t i = 0; i < b.rows.size(); ++i) k.rows[i] = b.rows[i];
    out.push_back(k);
  }
  return out;
}
}  // namespace
std::vector<KStep> uniform_ksteps(const finrom_rom_desc* a, const std::vector<int>& order, int rule) {
  std::vector<KStep> ksteps;
  auto pattern = [&](int row) { return std::vector<int>(a->term_p + a->row_ptr[row], a->term_p + a->row_ptr[row + 1]); };
  std::vector<int> byp(order);
  std::stable_sort(byp.begin(), byp.end(), [&](int x, int y) { return pattern(x) < pattern(y); });
  LeftClasses left;
  for (size_t i0 = 0; i0 < byp.size();) {
    size_t i1 = i0;
    while (i1 < byp.size() && pattern(byp[i1]) == pattern(byp[i0])) ++i1;
    size_t i = i0;
    for (; i + 4 <= i1; i += 4) ksteps.push_back({pattern(byp[i]), {byp[i], byp[i + 1], byp[i + 2], byp[i + 3]}});
    if (i < i1) left.push_back({pattern(byp[i]), std::vector<int>(byp.begin() + i, byp.begin() + i1)});
    i0 = i1;
  }
  std::vector<KStep> packed = pack_consecutive(left);
  if (rule == PACK_FEWEST) {
    for (const std::vector<KStep>& cand : {pack_nested(left), pack_padded(left)})
      if (pack_cost(cand) < pack_cost(packed)) packed = cand;
  }
  ksteps.insert(ksteps.end(), packed.begin(), packed.end());
  std::stable_sort(ksteps.begin(), ksteps.end(), [](const KStep& x, const KStep& y) { return x.pat.size() > y.pat.size(); });
  return ksteps;
}

// ---- the same k-steps GROUPED by their leading parameter (proj_main_grouped, NB <= 5) ----------------------------------
// A k-step whose rows carry {theta_d} or {1, theta_d} belongs to group d and is accumulated DIVIDED by theta_d: its slab is
// T_d (no arithmetic at all) or T_d + (1/theta_d) T_0 (one multiply-add per block); the accumulators are rescaled where the
// group changes -- by (theta_d / theta_e)^2 between groups d and e, by theta_d^2 after the last -- so that the sum is the
// one the ungrouped loop forms, up to rounding.  Everything else (rows that touch two parameters, merged leftovers) comes
// first, at scale 1, with the usual coefficients.  The per-sample scalars (1, theta, 1 / theta, the rescale factors) are
// one row of RomDev::ext, filled by rom_ext_kernel ahead of the projection kernel; the records name them by index.
// kclass (the half list of a mirror-symmetric ROM, DESIGN 4b'): per k-step 0 = rows that count twice (left of the symmetry line),
// 1 = rows that count once (on it).  The k-steps that count twice all come first; the factor of the record that opens the first
// k-step that counts once -- or the final factor if there is none -- carries an exact 2 (bit 1 of its ext_def flags), so the
// weights act on the accumulators and no row is scaled by sqrt(2).  slot0 / ext0: the list's rows and factors sit behind
// another list's (slot0 table slots, ext0 scalars, of which the first 1 + 2 P are shared); `def` then holds the factors only.
// scale_free (the short half list, group_pays above): a leading parameter whose group would not pay for its rescale stays at scale 1;
// what is left of the factors is the exact 2 where the weight class changes and the final one.
bool build_grouped_tables(const finrom_rom_desc* a, const std::vector<KStep>& ksteps, int rp, GroupedTables& out,
                          const std::vector<int>* kclass, int slot0, int ext0, bool scale_free) {
  const int r = a->r;
  struct GStep { int cls, group; std::vector<int> pat; const int* rows; };
  std::vector<GStep> gs;
  for (size_t k = 0; k < ksteps.size(); ++k) {
    const KStep& ks = ksteps[k];
    if (ks.rows[0] < 0 && ks.rows[1] < 0 && ks.rows[2] < 0 && ks.rows[3] < 0) continue;      // (padding k-steps of the ungrouped list)
    int group = 0;
    std::vector<int> pat = ks.pat;
    if (pat.size() == 1 && pat[0] != 0) group = pat[0];
    else if (pat.size() == 2 && (pat[0] == 0) != (pat[1] == 0)) { group = pat[0] ? pat[0] : pat[1]; pat = {group, 0}; }
    gs.push_back({kclass ? (*kclass)[k] : 0, group, pat, ks.rows});
  }
  if (scale_free) {
    std::map<std::pair<int, int>, int> alone;      // (class, group) -> k-steps with the pattern {theta_group} alone
    for (const GStep& g : gs) if (g.group != 0 && g.pat.size() == 1) ++alone[{g.cls, g.group}];
    for (GStep& g : gs) {
      if (g.group == 0) continue;
      const auto it = alone.find({g.cls, g.group});
      if (group_pays(it == alone.end() ? 0 : it->second, rp / 16)) continue;
      if (g.pat.size() == 2) g.pat = {0, g.group};      // (T_0 first: `finish` then does fma(theta_d, T_d, T_0), NB operations)
      g.group = 0;
    }
  }
  std::stable_sort(gs.begin(), gs.end(), [](const GStep& x, const GStep& y) { return x.cls != y.cls ? x.cls < y.cls : x.group < y.group; });
  // segments: runs of one (class, group); segment 0 is the scale-1 start (group 0 of the first class, possibly empty)
  struct Seg { int cls, group; };
  std::vector<Seg> segs;
  bool any_group = false;
  if (!gs.empty()) segs.push_back({gs[0].cls, 0});
  for (const GStep& g : gs) {
    if (g.cls != segs.back().cls || g.group != segs.back().group) segs.push_back({g.cls, g.group});
    any_group = any_group || g.group != 0;
  }
  const int P = a->P, nfac = (int)segs.size(), base = ext0 ? ext0 : 1 + 2 * P, n_ext = base + nfac;
  if ((!any_group && !scale_free) || n_ext > 64) return false;      // (a scale-free list may have no group at all)
  // ext[0] = 1, ext[p] = theta_p, ext[P + p] = 1 / theta_p, then one factor per change of segment and the final one; as
  // (numerator, denominator, flags: 1 squared, 2 times two)
  std::vector<int> def(ext0 ? 0 : 3 * (size_t)base, 0);
  if (!ext0) for (int pp = 1; pp <= P; ++pp) { def[3 * pp] = pp; def[3 * (P + pp) + 1] = pp; }
  for (int g = 0; g < nfac; ++g) {      // factor g: from segment g to segment g + 1, the last one back to scale 1
    const bool last = g + 1 == nfac;
    const bool twice = kclass != nullptr && segs[g].cls == 0 && (last || segs[g + 1].cls == 1);
    def.push_back(segs[g].group); def.push_back(last ? 0 : segs[g + 1].group); def.push_back(1 | (twice ? 2 : 0));
  }
  std::vector<double>& tvg = out.tvg; std::vector<int>& kmg = out.kmg;
  tvg.clear(); kmg.clear();
  int slot = slot0, seg = 0;
  bool first = true;
  for (const GStep& g : gs) {
    const int nt = (int)g.pat.size();
    int rec[8] = {slot, nt, 0, 0, 0, 0, 0, 0};
    for (int t = 0; t < nt; ++t) rec[4 + t] = g.group ? (t == 0 ? 0 : P + g.group) : g.pat[t];
    if (rec[4] == 0) rec[2] |= 1;                       // the first coefficient is 1: its rows are the slab as they are
    if (g.cls != segs[seg].cls || g.group != segs[seg].group) {
      ++seg;
      if (!first) { rec[2] |= 2; rec[3] = base + seg - 1; }      // (nothing to rescale in front of the very first k-step)
    }
    first = false;
    kmg.insert(kmg.end(), rec, rec + 8);
    for (int t = 0; t < nt; ++t)
      for (int q = 0; q < 4; ++q) {
        const size_t base_ = tvg.size();
        tvg.resize(base_ + rp, 0.0);
        const int row = g.rows[q];
        if (row < 0) continue;
        for (int tt = a->row_ptr[row]; tt < a->row_ptr[row + 1]; ++tt)
          if (a->term_p[tt] == g.pat[t]) for (int col = 0; col < r; ++col) tvg[base_ + col] += a->term_val[(size_t)tt * r + col];
      }
    slot += nt;
  }
  // zero k-steps fill the list up to a multiple of three (the loop rotates three slab buffers) and serve the pipeline's reads
  // of the records / rows of the k-steps behind the last one
  int nkg = (int)gs.size();
  const int zslot = slot;
  tvg.resize(tvg.size() + (size_t)4 * 4 * rp, 0.0);
  while (nkg % 3) { int rec[8] = {zslot, 1, 1, 0, 0, 0, 0, 0}; kmg.insert(kmg.end(), rec, rec + 8); ++nkg; }
  for (int k = 0; k < 8; ++k) { int rec[8] = {zslot, 1, 1, 0, 0, 0, 0, 0}; kmg.insert(kmg.end(), rec, rec + 8); }
  out.def = def; out.nkg = nkg; out.n_ext = n_ext; out.ext_final = base + nfac - 1;
  out.live = (int)gs.size(); out.fma_ksteps = 0;
  for (const GStep& g : gs) out.fma_ksteps += kstep_vector_ops(g.pat, g.group == 0) > 0;
  return true;
}

// ---- the half descriptor of a mirror-symmetric ROM (finrom_rom_set_mirror) -------------------------------------------------
int validate_rom_mirror(const finrom_rom_desc* a, int n_full, const int32_t* row_node, const double* row_weight, const int32_t* theta_twin) {
  if (!a || !row_node || !row_weight || !theta_twin) { set_error("rom_mirror: null argument"); return FINROM_ERR_ARG; }
  if (int rc = validate_rom_desc(a)) return rc;
  if (a->n > n_full) { set_error("rom_mirror: more half rows than rows"); return FINROM_ERR_ARG; }
  for (int p = 0; p < a->P; ++p)
    if (theta_twin[p] < 0 || theta_twin[p] >= a->P || theta_twin[theta_twin[p]] != p) { set_error("rom_mirror: theta_twin is not an involution"); return FINROM_ERR_ARG; }
  std::vector<char> seen((size_t)n_full, 0);
  int64_t covered = 0;
  for (int i = 0; i < a->n; ++i) {
    // (with the row's other checks, not validate_row_weights up front: a descriptor wrong in two ways reports what it always did)
    if (row_weight[i] != 1.0 && row_weight[i] != 2.0) { set_error("rom_mirror: a row weight is neither 1 nor 2"); return FINROM_ERR_ARG; }
    if (row_node[i] < 0 || row_node[i] >= n_full) { set_error("rom_mirror: row_node out of range"); return FINROM_ERR_ARG; }
    if (seen[row_node[i]]) { set_error("rom_mirror: a row is listed twice"); return FINROM_ERR_ARG; }
    seen[row_node[i]] = 1;
    covered += row_weight[i] == 2.0 ? 2 : 1;
  }
  if (covered != n_full) { set_error("rom_mirror: the weights do not add up to the number of rows"); return FINROM_ERR_ARG; }
  // only one parameter of a mirror pair may appear (the samples that walk this list carry the same value in both)
  unsigned used = 0;
  for (int t = 0; t < a->nterms; ++t) if (a->term_p[t] > 0) used |= 1u << (a->term_p[t] - 1);
  for (int p = 0; p < a->P; ++p)
    if (theta_twin[p] != p && (used & (1u << p)) && (used & (1u << theta_twin[p]))) { set_error("rom_mirror: both parameters of a mirror pair appear"); return FINROM_ERR_ARG; }
  return 0;
}

// the half list's k-steps: rows that count twice and rows that count once never share a k-step.  A descriptor with rows that have no
// terms is the SHORT list (engine.py: mirror_skip_rows dropped them): its leftovers are packed for the fewest k-steps (PACK_FEWEST);
// a descriptor without such rows keeps the list it always had.
std::vector<KStep> mirror_ksteps(const finrom_rom_desc* a, const double* row_weight, std::vector<int>& kclass) {
  std::vector<KStep> ksteps;
  kclass.clear();
  const std::vector<int> order = rows_by_term_count(a);
  const int rule = (int)order.size() < a->n ? PACK_FEWEST : PACK_CONSECUTIVE;
  for (int cls = 0; cls < 2; ++cls) {
    std::vector<int> part;
    for (int row : order) if ((row_weight[row] == 2.0) == (cls == 0)) part.push_back(row);
    for (const KStep& ks : uniform_ksteps(a, part, rule)) { ksteps.push_back(ks); kclass.push_back(cls); }
  }
  return ksteps;
}
// the short half list (a descriptor with term-less rows) is built scale-free unless the A/B switch asks for the groups it had
bool env_rom_short_grouped() { return getenv("FINROM_ROM_SHORT_GROUPED") != nullptr; }
bool short_scale_free(const finrom_rom_desc* a, bool short_grouped) { return !short_grouped && (int)rows_by_term_count(a).size() < a->n; }

// ---- the compact list (finrom_rom_set_mirror_compact, DESIGN 4b''): the rows of a pattern class rotated onto their singular directions
// One-sided Jacobi on the ROWS of M [m x w] (Hestenes): plane rotations of row pairs until every pair is orthogonal to rounding,
// relative to the two rows' own sizes -- so directions 1e-10 of the largest come out with their digits, which the class Gram
// matrix (1e-20, below rounding) could not give.  Q [m x m] takes the same rotations from the identity: M_out = Q M_in.  Then
// rows by size, descending: sigma[i] = |row i|.
static void jacobi_rows(std::vector<double>& M, int m, int w, std::vector<double>& Q, std::vector<double>& sigma) {
  Q.assign((size_t)m * m, 0.0);
  for (int i = 0; i < m; ++i) Q[(size_t)i * m + i] = 1.0;
  auto dot = [&](const double* x, const double* y) { double s = 0.0; for (int k = 0; k < w; ++k) s += x[k] * y[k]; return s; };
  auto rotate = [](double* x, double* y, int len, double c, double s) {
    for (int k = 0; k < len; ++k) { const double a = x[k], b = y[k]; x[k] = c * a - s * b; y[k] = s * a + c * b; }
  };
  constexpr double kTol = 4.0 * 2.220446049250313e-16;
  for (int sweep = 0; sweep < 60; ++sweep) {
    bool any = false;
    for (int i = 0; i < m; ++i)
      for (int j = i + 1; j < m; ++j) {
        double* x = &M[(size_t)i * w]; double* y = &M[(size_t)j * w];
        const double a = dot(x, x), b = dot(y, y), g = dot(x, y);
        if (g == 0.0 || std::fabs(g) <= kTol * std::sqrt(a) * std::sqrt(b)) continue;
        any = true;
        const double zeta = (b - a) / (2.0 * g), t = (zeta >= 0.0 ? 1.0 : -1.0) / (std::fabs(zeta) + std::sqrt(1.0 + zeta * zeta));
        const double c = 1.0 / std::sqrt(1.0 + t * t), s = c * t;
        rotate(x, y, w, c, s);
        rotate(&Q[(size_t)i * m], &Q[(size_t)j * m], m, c, s);
      }
    if (!any) break;
  }
  std::vector<double> nrm(m);
  for (int i = 0; i < m; ++i) nrm[i] = std::sqrt(dot(&M[(size_t)i * w], &M[(size_t)i * w]));
  std::vector<int> ord(m);
  for (int i = 0; i < m; ++i) ord[i] = i;
  std::stable_sort(ord.begin(), ord.end(), [&](int x, int y) { return nrm[x] > nrm[y]; });
  std::vector<double> Ms(M.size()), Qs(Q.size());
  sigma.resize(m);
  for (int i = 0; i < m; ++i) {
    std::memcpy(&Ms[(size_t)i * w], &M[(size_t)ord[i] * w], w * sizeof(double));
    std::memcpy(&Qs[(size_t)i * m], &Q[(size_t)ord[i] * m], m * sizeof(double));
    sigma[i] = nrm[ord[i]];
  }
  M.swap(Ms); Q.swap(Qs);
}

}  // namespace finrom

using namespace finrom;

// what finrom_rom_grouped_tables and finrom_rom_mirror_tables hand back: the sizes, and the tables where the caller gave room
// (g == nullptr: the descriptor has no grouped form -- all sizes 0, nothing written)
static int copy_out_tables(const GroupedTables* g, int rp, int32_t* nkg, int32_t* n_ext, int32_t* ext_final, int64_t* n_slots,
                           int32_t* kmg, double* tvg, int32_t* ext_def) {
  if (!g) { *nkg = 0; *n_ext = 0; *ext_final = 0; *n_slots = 0; return 0; }
  *nkg = g->nkg; *n_ext = g->n_ext; *ext_final = g->ext_final; *n_slots = (int64_t)(g->tvg.size() / ((size_t)4 * rp));
  if (kmg) std::memcpy(kmg, g->kmg.data(), g->kmg.size() * sizeof(int));
  if (tvg) std::memcpy(tvg, g->tvg.data(), g->tvg.size() * sizeof(double));
  if (ext_def) std::memcpy(ext_def, g->def.data(), g->def.size() * sizeof(int));
  return 0;
}

extern "C" {

// Host only (no device needed): the grouped tables finrom_rom_create builds for r <= 80, for tests of the host logic.
int finrom_rom_grouped_tables(const finrom_rom_desc* a, int32_t* nkg, int32_t* n_ext, int32_t* ext_final, int64_t* n_slots,
                              int32_t* kmg, double* tvg, int32_t* ext_def) {
  if (!a || !nkg || !n_ext || !ext_final || !n_slots) { set_error("rom_grouped_tables: null argument"); return FINROM_ERR_ARG; }
  if (int rc = validate_rom_desc(a)) return rc;
  const int NB = (a->r + 15) / 16, rp = 16 * NB;
  GroupedTables g;
  const bool grouped = NB <= 5 && build_grouped_tables(a, uniform_ksteps(a, rows_by_term_count(a)), rp, g);
  return copy_out_tables(grouped ? &g : nullptr, rp, nkg, n_ext, ext_final, n_slots, kmg, tvg, ext_def);
}

int finrom_rom_mirror_validate(const finrom_rom_desc* a, int32_t n_full, const int32_t* row_node, const double* row_weight,
                               const int32_t* theta_twin) {
  return validate_rom_mirror(a, n_full, row_node, row_weight, theta_twin);
}

// Host only: the half list finrom_rom_set_mirror builds from the half descriptor, as a list of its own (slots and scalars from 0).
int finrom_rom_mirror_tables(const finrom_rom_desc* a, const double* row_weight, int32_t* nkg, int32_t* n_ext, int32_t* ext_final,
                             int64_t* n_slots, int32_t* kmg, double* tvg, int32_t* ext_def) {
  if (!a || !row_weight || !nkg || !n_ext || !ext_final || !n_slots) { set_error("rom_mirror_tables: null argument"); return FINROM_ERR_ARG; }
  if (int rc = validate_rom_desc(a)) return rc;
  if (int rc = validate_row_weights(a, row_weight)) return rc;
  const int NB = (a->r + 15) / 16, rp = 16 * NB;
  GroupedTables g;
  std::vector<int> kclass;
  const std::vector<KStep> ksteps = mirror_ksteps(a, row_weight, kclass);
  const bool grouped = NB <= 5 && build_grouped_tables(a, ksteps, rp, g, &kclass, 0, 0, short_scale_free(a, env_rom_short_grouped()));
  return copy_out_tables(grouped ? &g : nullptr, rp, nkg, n_ext, ext_final, n_slots, kmg, tvg, ext_def);
}

// Host only: what the half list of this descriptor multiplies -- rows with terms, k-steps before the padding to a multiple of three,
// and how many of those need vector arithmetic (0, 0, 0 where finrom_rom_mirror_tables reports no grouped form).
int finrom_rom_mirror_counts(const finrom_rom_desc* a, const double* row_weight, int32_t* live_rows, int32_t* ksteps, int32_t* fma_ksteps) {
  if (!a || !row_weight || !live_rows || !ksteps || !fma_ksteps) { set_error("rom_mirror_counts: null argument"); return FINROM_ERR_ARG; }
  if (int rc = validate_rom_desc(a)) return rc;
  if (int rc = validate_row_weights(a, row_weight)) return rc;
  const int NB = (a->r + 15) / 16, rp = 16 * NB;
  GroupedTables g;
  std::vector<int> kclass;
  const std::vector<KStep> ks = mirror_ksteps(a, row_weight, kclass);
  *live_rows = 0; *ksteps = 0; *fma_ksteps = 0;
  if (NB > 5 || !build_grouped_tables(a, ks, rp, g, &kclass, 0, 0, short_scale_free(a, env_rom_short_grouped()))) return 0;
  *live_rows = (int32_t)rows_by_term_count(a).size(); *ksteps = g.live; *fma_ksteps = g.fma_ksteps;
  return 0;
}

// Host only: the rows of the COMPACT list from a short descriptor (DESIGN 4b'').  Every row's terms are multiplied by sqrt(weight)
// and its load divided by it (desc->rhs is weight F: psi^T rhs stays what it was), so the result has no weight classes.  The
// unloaded rows with terms form a class per pattern; a class's stacked tables [T_p1 | T_p2 | ..] are orthogonalised by
// jacobi_rows, and where leaving out the rotated rows below tau x (the largest singular value over all classes) saves a k-step
// of four rows the class's rows are REPLACED by the rotated ones, largest first, in the class's row positions.  Out: term_val
// [nterms x r] and rhs [n] of the compact descriptor (same row_ptr / term_p), row_class [n] (-1: loaded or term-less), row_sigma
// [n] (the singular values of the row's class in its row positions, largest first, rotated or not; 0 outside classes),
// row_keep [n] (0: a rotated row below the threshold -- the caller gives it no terms), Q (optional, [n x q_ld], q_ld >= the
// largest class): row i of a ROTATED class is  sum_j Q[i][j] sqrt(w_j) (member j's row),  members in ascending row order.
int finrom_rom_compact_rows(const finrom_rom_desc* a, const double* row_weight, double tau, double* term_val, double* rhs,
                            int32_t* row_class, double* row_sigma, int32_t* row_keep, double* Q, int32_t q_ld, double* sigma_max) {
  if (!a || !row_weight || !term_val || !rhs || !row_class || !row_sigma || !row_keep || !sigma_max) { set_error("rom_compact_rows: null argument"); return FINROM_ERR_ARG; }
  if (int rc = validate_rom_desc(a)) return rc;
  if (int rc = validate_row_weights(a, row_weight)) return rc;
  if (!a->rhs || !(tau >= 0.0 && tau < 1.0)) { set_error("rom_compact_rows: need the load and 0 <= tau < 1"); return FINROM_ERR_ARG; }
  const int r = a->r, n = a->n;
  for (int i = 0; i < n; ++i) {
    const double sw = std::sqrt(row_weight[i]);
    rhs[i] = a->rhs[i] / sw; row_class[i] = -1; row_sigma[i] = 0.0; row_keep[i] = 1;
    for (int t = a->row_ptr[i]; t < a->row_ptr[i + 1]; ++t)
      for (int col = 0; col < r; ++col) term_val[(size_t)t * r + col] = sw * a->term_val[(size_t)t * r + col];
  }
  std::map<std::vector<int>, std::vector<int>> classes;      // pattern -> its unloaded rows, ascending
  for (int i = 0; i < n; ++i)
    if (a->row_ptr[i + 1] > a->row_ptr[i] && a->rhs[i] == 0.0)
      classes[std::vector<int>(a->term_p + a->row_ptr[i], a->term_p + a->row_ptr[i + 1])].push_back(i);
  struct Rot { const std::vector<int>* rows; int nt; std::vector<double> M, Qc, sigma; };
  std::vector<Rot> rots;
  *sigma_max = 0.0;
  for (const auto& c : classes) {
    Rot x{&c.second, (int)c.first.size(), {}, {}, {}};
    const int m = (int)c.second.size(), w = x.nt * r;
    if (Q && m > q_ld) { set_error("rom_compact_rows: q_ld is smaller than the largest class"); return FINROM_ERR_ARG; }
    x.M.resize((size_t)m * w);
    for (int j = 0; j < m; ++j) std::memcpy(&x.M[(size_t)j * w], term_val + (size_t)a->row_ptr[c.second[j]] * r, w * sizeof(double));
    jacobi_rows(x.M, m, w, x.Qc, x.sigma);
    *sigma_max = std::max(*sigma_max, x.sigma[0]);
    rots.push_back(std::move(x));
  }
  if (Q) std::fill(Q, Q + (size_t)n * q_ld, 0.0);
  for (size_t ci = 0; ci < rots.size(); ++ci) {
    const Rot& x = rots[ci];
    const std::vector<int>& rows = *x.rows;
    const int m = (int)rows.size(), w = x.nt * r;
    int kept = 0;
    for (int j = 0; j < m; ++j) kept += x.sigma[j] >= tau * *sigma_max;
    const bool rotate = (kept + 3) / 4 < (m + 3) / 4;      // (only where it saves a k-step: the rotated rows are dense in the class)
    for (int j = 0; j < m; ++j) {
      row_class[rows[j]] = (int32_t)ci; row_sigma[rows[j]] = x.sigma[j];
      if (!rotate) continue;
      row_keep[rows[j]] = x.sigma[j] >= tau * *sigma_max;
      std::memcpy(term_val + (size_t)a->row_ptr[rows[j]] * r, &x.M[(size_t)j * w], w * sizeof(double));
      if (Q) std::memcpy(Q + (size_t)rows[j] * q_ld, &x.Qc[(size_t)j * m], m * sizeof(double));
    }
  }
  return 0;
}

}  // extern "C"
