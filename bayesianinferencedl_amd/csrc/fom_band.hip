// FOM throughput path: frontal band sweep with the front in REGISTERS (lane = sample).
//
// Replaces, for a whole batch, Fin.forward + Fin.qoi_operator (fom/forward_solve.py:270-291, 408-412) like the schedule
// interpreter of fom_kernels.hip does, but without keeping the factor's working set in HBM.  The fin is a long thin domain:
// ordered fin by fin (tip -> root, column by column) and then up the post row by row, the Cholesky factorisation only ever
// touches a window of NS = B + 1 consecutive nodes (B = half bandwidth: m/4 + 1 in a fin, m + 1 in the post), i.e. a
// triangle of NS (NS + 1) / 2 values per sample -- 105 doubles at m = 12.  That triangle lives in VGPRs; the window slides by
// renaming slots cyclically (node t sits in slot t mod NS), and the loop over pivots is unrolled NS times so that every
// register index is a compile-time constant.  Per pivot: 1/sqrt, B multiplies, B (B + 1) / 2 multiply-adds, B + 2 coalesced
// 512-B stores (the finished column of L, 1/L_jj, y_j) -- no operand fetches.  The backward substitution streams the
// columns back once.  HBM traffic per sample: the assembled entries (3 per node) + 2 x the factor; the interpreter moves
// 5-6 x as much and executes ~14 instructions per multiply-add.
//
// Irregularity (bayesianinferencedl_amd/bandplan.py): eliminating a fin couples its interface nodes, which sit in
// consecutive post ROWS; couplings that span more than B positions make the far node an *extra* front member.  Extras live
// in LDS (their coupling to each window slot, diagonal, right-hand side, mutual couplings); a table says, per pivot, which
// extra slots take part, and an extra is folded into the register window when its node enters it.  <= 4 alive at m = 12.
//
// All tables are wave-uniform and read with scalar loads; every index is validated on the host in finrom_fom_set_band.
#include "fom_band_device.h"

namespace finrom {

namespace {

// ---- forward: factorisation fused with L y = F over one segment ----------------------------------------------------------
// (PF: the right-hand side of the entering node travels with its three matrix entries -- for callers that run one wave per SIMD
// or less, where nothing else hides the load; the m <= 12 kernel is HBM-bound and keeps its register budget)
// (NOSTORE: the QoI-only form below -- nothing of the segment's factor or y leaves the registers)
// (NF > 0, the post with NOSTORE: the observation rows as functionals.  With c_o the weights of row o on the post -- its post-only
// part plus, on the interface nodes of its fin, the g that the fin's sweep left -- the observable is
//     q_o = c_o^T A_post^-1 f = (L^-1 c_o)^T (L^-1 f),
// so c_o rides the sweep as one more right-hand side: window fs->zw[o] beside yw, an LDS slot per extra beside XY (at XL::SIZE),
// and q_o gathers z_p y_p pivot by pivot.  No column of L, no y, no coupling to an extra is stored and no backward sweep follows.)
template <int NS, bool POST, int NXM, bool PF = false, bool NOSTORE = false, int NF = 0>
__device__ __forceinline__ void band_sweep(const BandDev& p, const Io& io, double* __restrict__ xs, const double* __restrict__ Fg,
                                           const int* __restrict__ abmap, const PostTables& T, int g0, int e0, int npiv, int ntot, int L0,
                                           double (&win)[NS * (NS + 1) / 2], double (&yw)[NS], int& bad,
                                           FnState<(NF > 0 ? NF : 1), NS>* __restrict__ fs = nullptr) {
  constexpr int B = NS - 1;
  using L = XL<NS, NXM>;
  constexpr int XZ = L::SIZE;                            // NF > 0: the extras' carried functional values, [NXM][NF]
  static_assert(NF == 0 || (POST && NOSTORE && !PF), "the functional windows belong to the post's store-free sweep");
  static_for<0, NS*(NS + 1) / 2>([&](auto i) { win[decltype(i)::value] = 0.0; });
  static_for<0, NS>([&](auto i) { yw[decltype(i)::value] = 0.0; });
  if constexpr (POST) static_for<0, L::SIZE + NXM * NF>([&](auto i) { xs[decltype(i)::value * 64] = 0.0; });
  if constexpr (NF > 0) static_for<0, NF>([&](auto oc) {
    constexpr int o = decltype(oc)::value;
    fs->q[o] = 0.0;
    static_for<0, NS>([&](auto i) { fs->zw[o][decltype(i)::value] = 0.0; });
  });

  // node t enters the window in slot u = t mod NS (the slot its predecessor t - NS has just left)
  auto enter = [&](auto uc, int t, double ab0, double ab1, double ab2, double fpre = 0.0) {
    constexpr int u = decltype(uc)::value;
    static_for<0, NS>([&](auto vc) { constexpr int v = decltype(vc)::value; if constexpr (v != u) win[tri(u, v)] = 0.0; });
    double diag = 0.0, yv = 0.0;
    double zv[NF > 0 ? NF : 1];
    if constexpr (NF > 0) {                              // c_o[t]: the row's own weight, plus its fin's g where t is an interface node
      const int row = fs->T.piv_row[t];
      double gv = 0.0;
      if (row >= 0) gv = io.ld(p.offY + fs->T.piv_off[t]);
      static_for<0, NF>([&](auto oc) { constexpr int o = decltype(oc)::value; zv[o] = fs->T.cw[t * NF + o] + (row == o ? gv : 0.0); });
    }
    if constexpr (POST) {
      static_for<0, NXM>([&](auto sc) { xs[(L::X + decltype(sc)::value * NS + u) * 64] = 0.0; });
      const int ex = T.ent_extra[t];
      if (ex != 0) {                                     // the node was an extra: its state moves from LDS into the window
        const int sl = ex - 1;
        if constexpr (NF > 0) static_for<0, NF>([&](auto oc) {
          constexpr int o = decltype(oc)::value;
          zv[o] = xs[(XZ + sl * NF + o) * 64] + zv[o];
          xs[(XZ + sl * NF + o) * 64] = 0.0;
        });
        static_for<0, NS>([&](auto vc) {
          constexpr int v = decltype(vc)::value;
          if constexpr (v != u) win[tri(u, v)] = xs[(L::X + sl * NS + v) * 64];
        });
        diag = xs[(L::XD + sl) * 64]; yv = xs[(L::XY + sl) * 64];
        static_for<0, NXM>([&](auto oc) {                // its couplings to the other extras become their window couplings
          constexpr int o = decltype(oc)::value;
          if (o != sl) {
            const int a = o > sl ? o : sl, b = o > sl ? sl : o;
            const int idx = L::XX + a * (a - 1) / 2 + b;
            xs[(L::X + o * NS + u) * 64] = xs[idx * 64];
            xs[idx * 64] = 0.0;
          }
        });
        static_for<0, NS>([&](auto vc) { xs[(L::X + sl * NS + decltype(vc)::value) * 64] = 0.0; });
        xs[(L::XD + sl) * 64] = 0.0; xs[(L::XY + sl) * 64] = 0.0;
      }
    }
    win[tri(u, u)] = diag + ab0;
    win[tri(u, (u + NS - 1) % NS)] += ab1;               // previous node (zero entry where there is none)
    win[tri(u, (u + 1) % NS)] += ab2;                    // the node B positions back
    yw[u] = yv + (PF ? fpre : Fg[g0 + t]);
    if constexpr (NF > 0) static_for<0, NF>([&](auto oc) { fs->zw[decltype(oc)::value][u] = zv[decltype(oc)::value]; });
    if constexpr (POST) {
      for (int c = T.ecp_ptr[t], c1 = T.ecp_ptr[t + 1]; c < c1; ++c)       // long-range couplings of this node: to extras
        xs[(L::X + T.ecp_slot[c] * NS + u) * 64] += io.ld(T.ecp_off[c]);
    }
  };

  static_for<0, NS>([&](auto uc) {                       // prologue: the first NS nodes enter an empty window
    constexpr int u = decltype(uc)::value;
    if (u < ntot) {
      const int g = 3 * (g0 + u);
      enter(uc, u, io.ld(abmap[g]), io.ld(abmap[g + 1]), io.ld(abmap[g + 2]), PF ? Fg[g0 + u] : 0.0);
    }
  });

  // Main loop, software-pipelined: step s first eliminates pivot s - RF (whose entering node's three entries were requested RF
  // steps ago and sit in ring slot s mod RF), then requests the entries for pivot s into the slot it has just emptied.  RF
  // divides NS, so with the loop unrolled NS times ring slot and window slot are both compile-time constants.
  constexpr int RF = (NS % 2 == 0) ? 2 : NS;
  double ab[RF][3];
  double abf[PF ? RF : 1];
  int gq[3] = {0, 0, 0};                                 // PF: slot numbers / right-hand side for the NEXT step's requests
  double fq = 0.0;
  if constexpr (PF) {
    if (0 < npiv && NS < ntot) { const int g = 3 * (g0 + NS); gq[0] = abmap[g]; gq[1] = abmap[g + 1]; gq[2] = abmap[g + 2]; fq = Fg[g0 + NS]; }
  }
  static_for<0, RF>([&](auto i) { ab[decltype(i)::value][0] = ab[decltype(i)::value][1] = ab[decltype(i)::value][2] = 0.0; });
  for (int s0 = 0; s0 < npiv + RF; s0 += NS) {
    static_for<0, NS>([&](auto usc) {
      constexpr int us = decltype(usc)::value;
      constexpr int u = (us + NS - RF % NS) % NS;        // window slot of pivot s - RF
      constexpr int rs = us % RF;                        // ring slot (of pivot s - RF and, afterwards, of pivot s)
      const int sidx = s0 + us;
      const int pp = sidx - RF;
      if (pp >= 0 && pp < npiv) {
        const bool more = pp + NS < ntot;
        const double ab0 = ab[rs][0], ab1 = ab[rs][1], ab2 = ab[rs][2];
        const double d = win[tri(u, u)];
        if (!(d > 0.0)) bad = 1;
        double inv = __builtin_amdgcn_rsq(d);            // hardware estimate + two Newton steps (as the interpreter does)
        inv = inv * fma(-0.5 * d * inv, inv, 1.5);
        inv = inv * fma(-0.5 * d * inv, inv, 1.5);
        double l[NS];
        static_for<1, NS>([&](auto sc) { constexpr int s_ = decltype(sc)::value; l[s_] = win[tri((u + s_) % NS, u)] * inv; });
        const int base = p.offL + L0 + pp * NS;
        if constexpr (!NOSTORE) {
          static_for<1, NS>([&](auto sc) { constexpr int s_ = decltype(sc)::value; io.template stk<s_ - 1>(l[s_], base); });
          io.template stk<NS - 1>(inv, base);
        }
        const double yp = yw[u] * inv;
        if constexpr (!NOSTORE) io.st(yp, p.offY + e0 + pp);
        double zp[NF > 0 ? NF : 1];
        if constexpr (NF > 0) static_for<0, NF>([&](auto oc) {
          constexpr int o = decltype(oc)::value;
          zp[o] = fs->zw[o][u] * inv;
          fs->q[o] = fma(zp[o], yp, fs->q[o]);
          static_for<1, NS>([&](auto sc) {
            constexpr int s_ = decltype(sc)::value;
            fs->zw[o][(u + s_) % NS] = fma(-l[s_], zp[o], fs->zw[o][(u + s_) % NS]);
          });
        });
        static_for<1, NS>([&](auto sc) {
          constexpr int s_ = decltype(sc)::value;
          yw[(u + s_) % NS] = fma(-l[s_], yp, yw[(u + s_) % NS]);
          static_for<1, s_ + 1>([&](auto tc) {
            constexpr int t = decltype(tc)::value;
            win[tri((u + s_) % NS, (u + t) % NS)] = fma(-l[s_], l[t], win[tri((u + s_) % NS, (u + t) % NS)]);
          });
        });
        if constexpr (POST) {
          const int am = T.act[pp];
          if (am != 0) {
            double le[NXM];
            int k = 0;
            if constexpr (NF == 0) k = p.offLx + T.lx_ptr[pp];      // (the functional form has no lx_ptr: nothing is stored)
            static_for<0, NXM>([&](auto sc) {
              constexpr int sl = decltype(sc)::value;
              le[sl] = 0.0;
              if (am & (1 << sl)) {
                const double v = xs[(L::X + sl * NS + u) * 64] * inv;
                le[sl] = v;
                if constexpr (NF == 0) { io.st(v, k); ++k; }
                xs[(L::XY + sl) * 64] = fma(-v, yp, xs[(L::XY + sl) * 64]);
                if constexpr (NF > 0) static_for<0, NF>([&](auto oc) {
                  constexpr int a = (XZ + sl * NF + decltype(oc)::value) * 64;
                  xs[a] = fma(-v, zp[decltype(oc)::value], xs[a]);
                });
                xs[(L::XD + sl) * 64] = fma(-v, v, xs[(L::XD + sl) * 64]);
                static_for<1, NS>([&](auto tc) {
                  constexpr int t = decltype(tc)::value;
                  constexpr int a = (L::X + sl * NS + (u + t) % NS) * 64;
                  xs[a] = fma(-v, l[t], xs[a]);
                });
              }
            });
            static_for<1, NXM>([&](auto ac) {
              constexpr int a = decltype(ac)::value;
              static_for<0, a>([&](auto bc) {
                constexpr int b = decltype(bc)::value;
                xs[L::xx(a, b) * 64] = fma(-le[a], le[b], xs[L::xx(a, b) * 64]);
              });
            });
          }
        }
        if (more) enter(std::integral_constant<int, u>{}, pp + NS, ab0, ab1, ab2, PF ? abf[PF ? rs : 0] : 0.0);
        else {
          static_for<0, NS>([&](auto vc) { win[tri(u, decltype(vc)::value)] = 0.0; });      // nobody enters: the slot is empty
          if constexpr (NF > 0) static_for<0, NF>([&](auto oc) { fs->zw[decltype(oc)::value][u] = 0.0; });
        }
      }
      if (sidx < npiv && sidx + NS < ntot) {             // entries of the node that enters after pivot s: in flight for RF steps
        const int g = 3 * (g0 + sidx + NS);      // (physical slots: entries with the same affine record share one)
        if constexpr (PF) {                      // slot numbers and right-hand side were requested a step ago
          ab[rs][0] = io.ld(gq[0]); ab[rs][1] = io.ld(gq[1]); ab[rs][2] = io.ld(gq[2]);
          abf[rs] = fq;
        } else {
          ab[rs][0] = io.ld(abmap[g]); ab[rs][1] = io.ld(abmap[g + 1]); ab[rs][2] = io.ld(abmap[g + 2]);
        }
      }
      if constexpr (PF) {
        if (sidx + 1 < npiv && sidx + 1 + NS < ntot) {
          const int g = 3 * (g0 + sidx + 1 + NS);
          gq[0] = abmap[g]; gq[1] = abmap[g + 1]; gq[2] = abmap[g + 2]; fq = Fg[g0 + sidx + 1 + NS];
        }
      }
    });
  }
}

// ---- backward: L^T w = y over one segment (w overwrites y), pivots in reverse -------------------------------------------------
// ---- the post's sweep by WV waves that share the 64 samples of a workgroup (fom_band_ldsw_kernel) ----------------------------------
// One wave cannot keep more than 15 LDS instructions in flight (lgkmcnt), which left the one-wave LDS sweep at ~30 cycles per updated
// entry.  The update moves an entry ALONG ITS DIAGONAL (s, t) -> (s - 1, t - 1), so the triangle is split by diagonals d = s - t
// (snake order: equal entry counts) and no two waves ever touch the same entry.  Every wave reads the pivot column and derives
// 1/sqrt and the scaled column itself; the rest of a pivot is spread by role: wave ST stores the column of L and y, wave YU slides
// the right-hand-side window, wave E (the last one) owns the extras' state, the entering node and its prefetch pipeline.
// (First version, DESIGN 4a: the triangle in LDS, each wave reading its diagonals in bursts and writing them back one position
// up, two barriers per pivot: 8.5 -> 5.2 ms per 16k samples at m = 20.  band_sweep_ldsr below keeps the diagonals in registers.)
template <int WV> constexpr int diag_owner(int d) { const int r = d % (2 * WV); return r < WV ? r : 2 * WV - 1 - r; }
// (register variant: the last wave -- extras, entering node -- owns no diagonal; the update is cheap there, its own chain is not)
template <int WV> constexpr int diag_owner_r(int d) { return WV > 1 ? diag_owner<WV - 1>(d) : 0; }

// (registers) offsets of a wave's diagonals in its flat register array: diagonal d has B - d + 1 entries (t = 0 .. B - d)
template <int NS, int WV, int WVI> constexpr int dg_off(int d) {
  int o = 0;
  for (int e = 0; e < d; ++e) if (diag_owner_r<WV>(e) == WVI) o += NS - 1 - e + 1;
  return o;
}
template <int NS, int WV, int WVI> constexpr int dg_total() { return dg_off<NS, WV, WVI>(NS - 1); }

// LDS of the register variant, doubles per lane: 4 (NS + 1) exchange buffers | the extras' state up to XL::WX | the failure flag.
// ldsr_xrows: how many of the extras' NXM rows of NS fit into the 160 KB (320 doubles per lane) beside the rest
template <int NS, int NXM> constexpr int ldsr_xrows() {
  const int fixed = 4 * (NS + 1) + (XL<NS, NXM>::WX - NXM * NS) + 1, fit = (320 - fixed) / NS;
  return fit < NXM ? fit : NXM;
}
template <int NS, int NXM> constexpr int ldsr_state() { return 4 * (NS + 1) + XL<NS, NXM>::WX - (NXM - ldsr_xrows<NS, NXM>()) * NS; }   // = the flag's index

// ---- the same sweep with the triangle in the owners' REGISTERS ------------------------------------------------------------------
// The update moves an entry along its diagonal, and a diagonal belongs to one wave: the whole diagonal can live in that wave's
// registers (in place, ascending: plain register renaming), ~63 doubles per wave at NS = 22.  LDS then only carries what the waves
// hand to each other per pivot: the next pivot's column (each diagonal's first entry, published by its owner, + y_0) and the
// entering node's row (wave E) -- 2 x 23 + 2 x 23 doubles per lane, double-buffered, so ONE barrier per pivot -- instead of the
// 2 x 231 entry reads and writes of the update pass (which ran at LDS bandwidth: 1.5 of the sweep's 5 ms per 16k samples).
template <int NS, int NXM, int WV, int WVI>
__device__ __forceinline__ void band_sweep_ldsr(const BandDev& p, const Io& io, double* __restrict__ wl, const double* __restrict__ Fg,
                                                const int* __restrict__ abmap, const PostTables& T, int g0, int e0, int npiv, int ntot,
                                                int L0, int& bad) {
  constexpr int B = NS - 1, RS = NS + 1;
  constexpr int COL = 0, ROWB = 2 * RS, XOFF = 4 * RS;    // LDS (doubles per lane): COL[par][s | y_0] | ROWB[par][k | y_B] | the extras' state
  constexpr int ST = 0, YU = 1 % WV, E = WV - 1;
  using L = XL<NS, NXM>;
  // the extras' state (wave E only) sits in LDS now that the window has left it: a row update is ~50 LDS operations instead of
  // a round trip to L2 per extra.  Beyond NS = 22 the ten rows no longer fit beside the exchange buffers: the first
  // ldsr_xrows<NS, NXM>() rows stay in LDS, the others live in the workspace slice p.offX (same index), the scalars behind the
  // rows move down in LDS by the rows that left
  constexpr int XR = ldsr_xrows<NS, NXM>(), XSH = (NXM - XR) * NS;
  auto xld = [&](int idx) -> double { return wl[(XOFF + idx - XSH) * 64]; };                    // the scalars: XD, XY, XX
  auto xst = [&](double v, int idx) { wl[(XOFF + idx - XSH) * 64] = v; };
  auto xrld = [&](auto slc, int col) -> double {                                                // row slc (compile-time), slot col
    constexpr int sl = decltype(slc)::value;
    if constexpr (sl < XR) return wl[(XOFF + sl * NS + col) * 64]; else return io.ld(p.offX + sl * NS + col);
  };
  auto xrst = [&](double v, auto slc, int col) {
    constexpr int sl = decltype(slc)::value;
    if constexpr (sl < XR) wl[(XOFF + sl * NS + col) * 64] = v; else io.st(v, p.offX + sl * NS + col);
  };
  auto xrld_rt = [&](int sl, int col) -> double {                                               // (row known at run time only)
    if constexpr (XR == NXM) return wl[(XOFF + sl * NS + col) * 64];
    else return sl < XR ? wl[(XOFF + sl * NS + col) * 64] : io.ld(p.offX + sl * NS + col);
  };
  auto xrst_rt = [&](double v, int sl, int col) {
    if constexpr (XR == NXM) wl[(XOFF + sl * NS + col) * 64] = v;
    else { if (sl < XR) wl[(XOFF + sl * NS + col) * 64] = v; else io.st(v, p.offX + sl * NS + col); }
  };
  // LDS-only barrier: nothing a wave stores to the workspace inside this sweep is read by another wave before the sweep ends
  // (the caller's __syncthreads()), and __syncthreads() here would make every pivot wait for the column stores' acknowledgements
  auto barrier = [&]() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); };

  double corner = 0.0;                                   // window entry (B, 0) of the first pivot (wave E)
  // node t (renamed slot u) enters at position P of the window whose row-B buffer is `par` (wave E only)
  auto enter = [&](auto pc, auto parc, auto proc, int t, int u, double ab0, double ab1, double ab2, int ex, int c0, int c1, double ft) {
    constexpr int P = decltype(pc)::value, par = decltype(parc)::value;
    constexpr bool PRO = decltype(proc)::value;       // prologue: into the LDS triangle; afterwards: the entering row's buffer
    double row[P + 1];
    static_for<0, P>([&](auto kc) { row[decltype(kc)::value] = 0.0; });
    double diag = 0.0, yv = 0.0;
    static_for<0, NXM>([&](auto sc) { xrst(0.0, sc, u); });
    if (ex != 0) {
      const int sl = ex - 1;
      static_for<0, P>([&](auto kc) {
        constexpr int k = decltype(kc)::value;
        int sk = u - P + k; sk += sk < 0 ? NS : 0;
        row[k] = xrld_rt(sl, sk);
      });
      diag = xld(L::XD + sl); yv = xld(L::XY + sl);
      double xo[NXM];
      static_for<0, NXM>([&](auto oc) {
        constexpr int o = decltype(oc)::value;
        const int a = o > sl ? o : sl, b = o > sl ? sl : o;
        xo[o] = (o != sl) ? xld(L::XX + a * (a - 1) / 2 + b) : 0.0;
      });
      static_for<0, NXM>([&](auto oc) {
        constexpr int o = decltype(oc)::value;
        if (o != sl) {
          const int a = o > sl ? o : sl, b = o > sl ? sl : o;
          xrst(xo[o], oc, u);
          xst(0.0, L::XX + a * (a - 1) / 2 + b);
        }
      });
      for (int v = 0; v < NS; ++v) xrst_rt(0.0, sl, v);
      xst(0.0, L::XD + sl); xst(0.0, L::XY + sl);
    }
    if constexpr (P >= 1) row[P - 1] += ab1;
    if constexpr (P == B) row[0] += ab2;
    static_for<0, P>([&](auto kc) { constexpr int k = decltype(kc)::value; wl[(ROWB + par * RS + k) * 64] = row[k]; });
    wl[(ROWB + par * RS + P) * 64] = diag + ab0;
    wl[(ROWB + par * RS + NS) * 64] = yv + ft;
    if constexpr (!PRO) wl[(COL + par * RS + B) * 64] = row[0];      // its coupling to the next pivot: the last entry of that pivot's column
    if constexpr (PRO && P == B) corner = row[0];
    for (int c = c0; c < c1; ++c) {
      const int sl = T.ecp_slot[c];
      xrst_rt(xrld_rt(sl, u) + io.ld(T.ecp_off[c]), sl, u);
    }
  };

  struct Tab { int am, lx, ex, c0, c1; double ft; };
  auto tables = [&](int q) -> Tab {
    Tab r{0, 0, 0, 0, 0, 0.0};
    if (q < npiv) {
      r.am = T.act[q]; r.lx = T.lx_ptr[q];
      if (q + NS < ntot) { const int t = q + NS; r.ex = T.ent_extra[t]; r.c0 = T.ecp_ptr[t]; r.c1 = T.ecp_ptr[t + 1]; r.ft = Fg[g0 + t]; }
    }
    return r;
  };
  auto slots = [&](int q, int (&gi)[3]) {
    if (q < npiv && q + NS < ntot) { const int g = 3 * (g0 + q + NS); gi[0] = abmap[g]; gi[1] = abmap[g + 1]; gi[2] = abmap[g + 2]; }
  };
  auto fetch = [&](int q, const int (&gi)[3], double (&ab)[3]) {
    if (q < npiv && q + NS < ntot) { ab[0] = io.ld(gi[0]); ab[1] = io.ld(gi[1]); ab[2] = io.ld(gi[2]); }
  };
  double abA[3] = {0.0, 0.0, 0.0}, abB[3] = {0.0, 0.0, 0.0};
  int giC[3] = {0, 0, 0};
  Tab cur{0, 0, 0, 0, 0, 0.0};
  // prologue: the first NS nodes enter one at a time; wave E forms the node's row (through the same buffer the main loop uses),
  // the owners of the diagonals pick their entries of it: (P, k) is entry k of diagonal P - k
  constexpr int DGT = dg_total<NS, WV, WVI>();
  double dg[DGT > 0 ? DGT : 1];
  static_for<0, (DGT > 0 ? DGT : 1)>([&](auto i) { dg[decltype(i)::value] = 0.0; });
  double yv[NS];
  static_for<0, NS>([&](auto sc) { yv[decltype(sc)::value] = 0.0; });
  if constexpr (WVI == E) {
    static_for<0, 4 * RS>([&](auto i) { wl[decltype(i)::value * 64] = 0.0; });
    for (int i = L::XD; i < L::WX; ++i) xst(0.0, i);
    for (int sl = 0; sl < NXM; ++sl) for (int v = 0; v < NS; ++v) xrst_rt(0.0, sl, v);
  }
  barrier();
  static_for<0, NS>([&](auto pc) {
    constexpr int P = decltype(pc)::value;
    if constexpr (WVI == E) {
      if (P < ntot) {
        const int g = 3 * (g0 + P);
        enter(pc, std::integral_constant<int, 0>{}, std::true_type{}, P, P, io.ld(abmap[g]), io.ld(abmap[g + 1]), io.ld(abmap[g + 2]),
              T.ent_extra[P], T.ecp_ptr[P], T.ecp_ptr[P + 1], Fg[g0 + P]);
      } else {
        static_for<0, RS>([&](auto kc) { wl[(ROWB + decltype(kc)::value) * 64] = 0.0; });
      }
    }
    barrier();
    static_for<0, P + 1>([&](auto kc) {
      constexpr int k = decltype(kc)::value, d_ = P - k;
      if constexpr (d_ < B) { if constexpr (diag_owner_r<WV>(d_) == WVI) dg[dg_off<NS, WV, WVI>(d_) + k] = wl[(ROWB + k) * 64]; }
    });
    if constexpr (WVI == YU) yv[P] = wl[(ROWB + NS) * 64];
    barrier();
  });
  if constexpr (WVI == E) {
    int giA[3] = {0, 0, 0}, giB[3] = {0, 0, 0};
    slots(0, giA); slots(1, giB); slots(2, giC);
    fetch(0, giA, abA); fetch(1, giB, abB);
    cur = tables(0);
    wl[(COL + B) * 64] = corner;                         // (ROWB[0] still holds row B and y_B: the first step appends them again)
  }
  static_for<0, B>([&](auto dc) {
    constexpr int d_ = decltype(dc)::value;
    if constexpr (diag_owner_r<WV>(d_) == WVI) wl[(COL + d_) * 64] = dg[dg_off<NS, WV, WVI>(d_)];
  });
  if constexpr (WVI == YU) wl[(COL + NS) * 64] = yv[0];
  barrier();
  int u = 0;
  auto step = [&](auto parc, int pp) {
    constexpr int par = decltype(parc)::value;
    Tab nxt{0, 0, 0, 0, 0, 0.0};
    int giD[3] = {0, 0, 0};
    const double d = wl[(COL + par * RS) * 64];
    if (!(d > 0.0)) bad = 1;
    double inv = __builtin_amdgcn_rsq(d);
    inv = inv * fma(-0.5 * d * inv, inv, 1.5);
    inv = inv * fma(-0.5 * d * inv, inv, 1.5);
    double l[NS];
    static_for<1, NS>([&](auto sc) { constexpr int s_ = decltype(sc)::value; l[s_] = wl[(COL + par * RS + s_) * 64] * inv; });
    const double yp = wl[(COL + par * RS + NS) * 64] * inv;
    // the node that entered with the previous pivot: its row is the last entry of every diagonal (written by wave E last step)
    static_for<0, B>([&](auto dc) {
      constexpr int d_ = decltype(dc)::value;
      if constexpr (diag_owner_r<WV>(d_) == WVI) dg[dg_off<NS, WV, WVI>(d_) + B - d_] = wl[(ROWB + par * RS + B - d_) * 64];
    });
    if constexpr (WVI == YU) yv[B] = wl[(ROWB + par * RS + NS) * 64];
    // (no barrier here: this pivot's results go to the OTHER column / row buffers)
    if constexpr (WVI == ST) {
      const int base = p.offL + L0 + pp * NS;
      static_for<1, NS>([&](auto sc) { constexpr int s_ = decltype(sc)::value; io.template stk<s_ - 1>(l[s_], base); });
      io.template stk<NS - 1>(inv, base);
      io.st(yp, p.offY + e0 + pp);
    }
    if constexpr (WVI == YU) {
      static_for<1, NS>([&](auto sc) { constexpr int s_ = decltype(sc)::value; yv[s_ - 1] = fma(-l[s_], yp, yv[s_]); });
      wl[(COL + (1 - par) * RS + NS) * 64] = yv[0];
    }
    static_for<0, B>([&](auto dc) {                      // own diagonals, in registers: one position up (in place, ascending)
      constexpr int d_ = decltype(dc)::value;
      if constexpr (diag_owner_r<WV>(d_) == WVI) {
        constexpr int off = dg_off<NS, WV, WVI>(d_);
        static_for<1, B - d_ + 1>([&](auto jc) { constexpr int j = decltype(jc)::value; dg[off + j - 1] = fma(-l[d_ + j], l[j], dg[off + j]); });
        wl[(COL + (1 - par) * RS + d_) * 64] = dg[off];     // the diagonal's entry of the next pivot's column
      }
    });
    // the scalar loads of the next pivots' table entries go HERE, behind this wave's last LDS read of the pivot: they share
    // lgkmcnt with LDS and return out of order, so the next wait for an LDS value also waits for them -- now the barrier's
    if constexpr (WVI == E) { nxt = tables(pp + 1); slots(pp + 3, giD); }
    if constexpr (WVI == E) {
      // extras with a non-zero coupling to this pivot, one after the other (requesting the rows of four of them together was not
      // faster here either: 5.36 vs 5.24 ms)
      const int am = cur.am;
      if (am != 0) {
        double le[NXM];
        int k = p.offLx + cur.lx;
        static_for<0, NXM>([&](auto sc) {
          constexpr int sl = decltype(sc)::value;
          le[sl] = 0.0;
          if (am & (1 << sl)) {
            double xv[NS];
            static_for<0, NS>([&](auto tc) {
              constexpr int t = decltype(tc)::value;
              int st_ = u + t; st_ -= st_ >= NS ? NS : 0;
              xv[t] = xrld(sc, st_);
            });
            const double xy = xld(L::XY + sl), xd = xld(L::XD + sl);
            const double v = xv[0] * inv;
            le[sl] = v;
            io.st(v, k); ++k;
            xst(fma(-v, yp, xy), L::XY + sl);
            xst(fma(-v, v, xd), L::XD + sl);
            static_for<1, NS>([&](auto tc) {
              constexpr int t = decltype(tc)::value;
              int st_ = u + t; st_ -= st_ >= NS ? NS : 0;
              xrst(fma(-v, l[t], xv[t]), sc, st_);
            });
          }
        });
        double xx[NXM * (NXM - 1) / 2];
        static_for<0, NXM*(NXM - 1) / 2>([&](auto ic) { xx[decltype(ic)::value] = xld(L::XX + decltype(ic)::value); });
        static_for<1, NXM>([&](auto ac) {
          constexpr int a = decltype(ac)::value;
          static_for<0, a>([&](auto bc) {
            constexpr int b = decltype(bc)::value;
            constexpr int i = a * (a - 1) / 2 + b;
            xst(fma(-le[a], le[b], xx[i]), L::XX + i);
          });
        });
      }
      if (pp + NS < ntot) enter(std::integral_constant<int, B>{}, std::integral_constant<int, 1 - par>{}, std::false_type{}, pp + NS, u,
                                abA[0], abA[1], abA[2], cur.ex, cur.c0, cur.c1, cur.ft);
      else {
        static_for<0, RS>([&](auto kc) { wl[(ROWB + (1 - par) * RS + decltype(kc)::value) * 64] = 0.0; });
        wl[(COL + (1 - par) * RS + B) * 64] = 0.0;
      }
      abA[0] = abB[0]; abA[1] = abB[1]; abA[2] = abB[2];
      fetch(pp + 2, giC, abB);
      giC[0] = giD[0]; giC[1] = giD[1]; giC[2] = giD[2];
      cur = nxt;
    }
    u = u + 1 == NS ? 0 : u + 1;
    barrier();
  };
#pragma unroll 1
  for (int pp = 0; pp < npiv; pp += 2) {
    step(std::integral_constant<int, 0>{}, pp);
    if (pp + 1 < npiv) step(std::integral_constant<int, 1>{}, pp + 1);
  }
}

// ---- QoI-only form (finrom_fom_solve / finrom_solve_pairs without w: the dataset loop, generate_fin_dataset.py:93-100) ------------
// The observables are linear functionals of w, and a fin's own nodes I are leaves of the elimination: with its interface nodes
// G on the post's side wall,   w_I = -A_II^-1 A_IG w_G   (the load is zero on the fins: checked when the plan is installed), so
//     b_I^T w_I + b_G^T w_G = (b_G - A_GI A_II^-1 b_I)^T w_G =: g^T w_G .
// g is what a forward sweep of the fin leaves in the right-hand-side window of its trailing (interface) nodes when the
// observation row's weights b ride along AS the right-hand side -- which is free, since the true right-hand side is zero there.
// The fin's columns of L, its y and its backward sweep are then never needed: 100 of the 266 KB per sample at m = 12 stay on
// the chip.  g (nif doubles per fin) waits in the fin's unused y region for the post's backward sweep to deliver w_G.
// Host side (engine.py::band_descriptor): FgQ = the observation weights on the fins' segment nodes and the load on the post's;
// the post-only remainder of B_obs as CSR; row_fin[o] = the fin whose functional belongs to row o (-1: none).
template <int NSF>
__device__ __forceinline__ void fin_functional_out(const BandDev& p, const Io& io, const double (&yw)[NSF], int f, int npiv, int stride) {
  for (int t = 0; t < p.nif; ++t) {
    const int su = (npiv + t) % NSF;
    double v = 0.0;
    static_for<0, NSF>([&](auto uc) { constexpr int u = decltype(uc)::value; v = su == u ? yw[u] : v; });
    io.st(v, p.offY + f * stride + t);
  }
}
// observable o from the post's w: the post-only part of the row + g^T w_G of the row's fin
__device__ __forceinline__ double qoi_row(const BandDev& p, const Io& io, const int* __restrict__ obs_ptr, const int* __restrict__ obs_idx,
                                          const double* __restrict__ obs_w, const int* __restrict__ row_fin,
                                          const int* __restrict__ iface_elim, int o, bool qo) {
  double q0 = 0.0, q1 = 0.0;
  const int t0 = obs_ptr[o], t1 = obs_ptr[o + 1];
  for (int t = t0; t < t1; t += 8) {                     // loads batched by 8
    double v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) v[u] = io.ld(p.offY + obs_idx[(t + u < t1) ? t + u : t1 - 1]);
#pragma unroll
    for (int u = 0; u < 8; u += 2) {
      q0 = fma((t + u < t1) ? obs_w[t + u] : 0.0, v[u], q0);
      q1 = fma((t + u + 1 < t1) ? obs_w[t + u + 1] : 0.0, v[u + 1], q1);
    }
  }
  if (qo) {
    const int f = row_fin[o];
    if (f >= 0)
      for (int t = 0; t < p.nif; ++t) q0 = fma(io.ld(p.offY + f * p.npf + t), io.ld(p.offY + iface_elim[f * p.nif + t]), q0);
  }
  return q0 + q1;
}

template <int NSF, int NSP, int NXM, bool QO>
__device__ __forceinline__ void fom_band_body(BandDev p, const int* __restrict__ abmap, const double* __restrict__ Fg,
                                                      const int* __restrict__ act,
                                                      const int* __restrict__ lx_ptr, const int* __restrict__ ent_extra,
                                                      const int* __restrict__ ecp_ptr, const int* __restrict__ ecp_slot,
                                                      const int* __restrict__ ecp_off, const int* __restrict__ schur_off,
                                                      const int* __restrict__ iface_elim, const int* __restrict__ obs_ptr,
                                                      const int* __restrict__ obs_idx, const double* __restrict__ obs_w,
                                                      const int* __restrict__ row_fin,
                                                      double* __restrict__ Gw, int64_t S, double* __restrict__ qoi,
                                                      int* __restrict__ info) {
  extern __shared__ __attribute__((aligned(16))) double xlds[];
  const int lane = threadIdx.x;
  const int64_t blk = blockIdx.x;
  double* __restrict__ Gs = Gw + blk * (int64_t)p.gsize * 64;
  Io io{__builtin_amdgcn_make_buffer_rsrc(Gs, 0, p.gsize * 512, 0x00020000), lane * 8};
  double* xs = xlds + lane;
  const PostTables T{act, lx_ptr, ent_extra, ecp_ptr, ecp_slot, ecp_off};
  int bad = 0;
  constexpr int NIFT = (NSF - 1) * NSF / 2;              // entries of a fin's Schur complement (q + 1 = NSF - 1 interface nodes)
  {
    double win[NSF * (NSF + 1) / 2], yw[NSF];
    for (int f = 0; f < p.nfins; ++f) {
      const int npiv = p.npf, ntot = p.npf + p.nif;
      band_sweep<NSF, false, NXM, false, QO>(p, io, xs, Fg, abmap, T, f * ntot, f * npiv, npiv, ntot, f * npiv * NSF, win, yw, bad);
      if constexpr (QO) fin_functional_out<NSF>(p, io, yw, f, npiv, npiv);
      // what is left in the window is the fin's Schur complement on its interface nodes: add it to their entries in the post
      int k = 0;
      for (int t = 0; t < p.nif; ++t)
        for (int s = 0; s <= t; ++s, ++k) {
          const int a = (npiv + t) % NSF, b = (npiv + s) % NSF;
          double v = 0.0;
          static_for<0, NSF>([&](auto ac) {
            static_for<0, decltype(ac)::value + 1>([&](auto bc) {
              constexpr int ua = decltype(ac)::value, ub = decltype(bc)::value;
              v = ((a == ua && b == ub) || (a == ub && b == ua)) ? win[tri(ua, ub)] : v;
            });
          });
          const int off = schur_off[f * NIFT + k];
          io.st(io.ld(off) + v, off);
        }
    }
  }
  {
    double win[NSP * (NSP + 1) / 2], yw[NSP];
    band_sweep<NSP, true, NXM>(p, io, xs, Fg, abmap, T, p.post_g0, p.post_e0, p.npost, p.npost, p.post_L0, win, yw, bad);
  }
  band_bsweep<NSP, true, NXM>(p, io, xs + XL<NSP, NXM>::WX * 64, T, nullptr, p.post_e0, p.npost, p.npost, p.post_L0, p.offY);
  if constexpr (!QO)
    for (int f = 0; f < p.nfins; ++f)
      band_bsweep<NSF, false, NXM>(p, io, xs, T, iface_elim + f * p.nif, f * p.npf, p.npf, p.npf + p.nif, f * p.npf * NSF, p.offY);

  const int64_t s = blk * 64 + lane;
  const double nanv = __builtin_nan("");
  if (bad) {                                             // not positive definite: NaN outputs and the flag, as the interpreter does
    if constexpr (!QO) for (int i = 0; i < p.n; ++i) io.st(nanv, p.offY + i);
    if (info != nullptr && s < S) atomicOr(&info[s], 1);
  }
  for (int o = 0; o < p.n_obs; ++o) {                    // QoI = B_obs w (fom :408-412)
    const double q = qoi_row(p, io, obs_ptr, obs_idx, obs_w, row_fin, iface_elim, o, QO);
    if (p.out_ptr != nullptr) {                          // half plan: each distinct row once, stored to all its output columns
      if (s < S)
        for (int c = p.out_ptr[o], c1 = p.out_ptr[o + 1]; c < c1; ++c) qoi[s * p.n_out + p.out_col[c]] = bad ? nanv : q;
    } else if (s < S) qoi[s * p.n_obs + o] = bad ? nanv : q;
  }
}

// ---- the half plan's QoI-only form with the post as functionals (DESIGN 4c') ------------------------------------------------------
// The fins as in fom_band_body<.., true>, except that a fin's g goes to nif slots of its own right behind the value slots (the
// workspace of this form is the value slots + nfins x nif doubles: BandDev::offY = nAB, finrom_fom_set_band_mirror); the post by
// band_sweep<.., NF>, after which the observables sit in registers.
template <int NSF, int NSP, int NXM, int NF>
__device__ __forceinline__ void fom_band_fn_body(BandDev p, const int* __restrict__ abmap, const double* __restrict__ Fg,
                                                 const int* __restrict__ act, const int* __restrict__ ent_extra,
                                                 const int* __restrict__ ecp_ptr, const int* __restrict__ ecp_slot,
                                                 const int* __restrict__ ecp_off, const int* __restrict__ schur_off,
                                                 const double* __restrict__ cw, const int* __restrict__ piv_row,
                                                 const int* __restrict__ piv_off, double* __restrict__ Gw, int64_t S,
                                                 double* __restrict__ qoi, int* __restrict__ info) {
  extern __shared__ __attribute__((aligned(16))) double xlds[];
  const int lane = threadIdx.x;
  const int64_t blk = blockIdx.x;
  double* __restrict__ Gs = Gw + blk * (int64_t)p.gsize * 64;
  Io io{__builtin_amdgcn_make_buffer_rsrc(Gs, 0, p.gsize * 512, 0x00020000), lane * 8};
  double* xs = xlds + lane;
  const PostTables T{act, nullptr, ent_extra, ecp_ptr, ecp_slot, ecp_off};
  int bad = 0;
  constexpr int NIFT = (NSF - 1) * NSF / 2;
  {
    double win[NSF * (NSF + 1) / 2], yw[NSF];
    for (int f = 0; f < p.nfins; ++f) {
      const int npiv = p.npf, ntot = p.npf + p.nif;
      band_sweep<NSF, false, NXM, false, true>(p, io, xs, Fg, abmap, T, f * ntot, f * npiv, npiv, ntot, f * npiv * NSF, win, yw, bad);
      fin_functional_out<NSF>(p, io, yw, f, npiv, p.nif);
      int k = 0;
      for (int t = 0; t < p.nif; ++t)
        for (int s = 0; s <= t; ++s, ++k) {
          const int a = (npiv + t) % NSF, b = (npiv + s) % NSF;
          double v = 0.0;
          static_for<0, NSF>([&](auto ac) {
            static_for<0, decltype(ac)::value + 1>([&](auto bc) {
              constexpr int ua = decltype(ac)::value, ub = decltype(bc)::value;
              v = ((a == ua && b == ub) || (a == ub && b == ua)) ? win[tri(ua, ub)] : v;
            });
          });
          const int off = schur_off[f * NIFT + k];
          io.st(io.ld(off) + v, off);
        }
    }
  }
  FnState<NF, NSP> fs;
  fs.T = BandFnDev{cw, piv_row, piv_off};
  {
    double win[NSP * (NSP + 1) / 2], yw[NSP];
    band_sweep<NSP, true, NXM, false, true, NF>(p, io, xs, Fg, abmap, T, p.post_g0, p.post_e0, p.npost, p.npost, p.post_L0, win, yw, bad, &fs);
  }
  const int64_t s = blk * 64 + lane;
  const double nanv = __builtin_nan("");
  if (bad && info != nullptr && s < S) atomicOr(&info[s], 1);
  if (s < S)
    static_for<0, NF>([&](auto oc) {                     // each distinct row once, stored to all its output columns
      constexpr int o = decltype(oc)::value;
      if (o < p.n_obs)
        for (int c = p.out_ptr[o], c1 = p.out_ptr[o + 1]; c < c1; ++c) qoi[s * p.n_out + p.out_col[c]] = bad ? nanv : fs.q[o];
    });
}

// ---- the same form on pivot records (DESIGN 4c'; BandFinRec / BandPostRec, finrom.h) -----------------------------------------------
// band_sweep reads, per pivot, nine wave-uniform tables where it needs them -- every read a scalar round trip on the critical path,
// with the address arithmetic of its table -- and loads the fin's g for an interface node behind a branch, whose join makes the
// wave wait for ALL its vector loads in every step: the entries requested for two steps ahead included.  Here a pivot's table
// values are one record, requested into SGPRs RF steps before they are used: at step s the node that enters behind pivot s has
//   its address part (three value slots and the slot of g, as byte offsets)   in ra[s mod RF] -- requested at step s - RF,
//   from which its values are requested into ab / gvr[s mod RF]               -- used at step s + RF,
//   and its enter part (ent_extra, act, ecp range, row, FgQ, cw) requested     -- into re[s mod RF], used at step s + RF.
// The load of g is unconditional (a node that is no interface node has a harmless slot in its record; the select on row == o
// discards it) and travels with the three entries.  Records are read through the constant address space (scalar loads, their
// waits at the uses) and requested at the END of a step, behind its last LDS access: scalar loads share lgkmcnt with LDS and return
// out of order, so any wait for an LDS value also waits for them.  The arithmetic is band_sweep<.., NOSTORE>'s, operation by
// operation: the results are the same bits.
typedef int rec_i4 __attribute__((ext_vector_type(4)));
typedef const rec_i4 __attribute__((address_space(4)))* rec_p;
__device__ __forceinline__ double rec_f64(int lo, int hi) { return __hiloint2double(hi, lo); }
__device__ __forceinline__ void rec_settle(rec_i4& v) {      // the wait for a requested part of a record happens where this stands
  int x = v.x, y = v.y, z = v.z, w = v.w;
  asm volatile("" : "+s"(x), "+s"(y), "+s"(z), "+s"(w));
  v = rec_i4{x, y, z, w};
}

template <int NS, bool POST, int NXM, int NF>
__device__ __forceinline__ void band_sweep_rec(const Io& io, double* __restrict__ xs, rec_p rec, const int* __restrict__ ecp_slot,
                                               const int* __restrict__ ecp_off, int npiv, int ntot, double (&win)[NS * (NS + 1) / 2],
                                               double (&yw)[NS], int& bad, FnState<(NF > 0 ? NF : 1), NS>* __restrict__ fs = nullptr) {
  using L = XL<NS, NXM>;
  constexpr int XZ = L::SIZE;
  constexpr int Q = POST ? sizeof(BandPostRec) / 16 : sizeof(BandFinRec) / 16;      // 16-byte loads per record; the first is the address part
  static_assert(POST == (NF > 0), "the post carries the functionals, the fins carry none");
  static_for<0, NS*(NS + 1) / 2>([&](auto i) { win[decltype(i)::value] = 0.0; });
  static_for<0, NS>([&](auto i) { yw[decltype(i)::value] = 0.0; });
  if constexpr (POST) static_for<0, L::SIZE + NXM * NF>([&](auto i) { xs[decltype(i)::value * 64] = 0.0; });
  if constexpr (NF > 0) static_for<0, NF>([&](auto oc) {
    constexpr int o = decltype(oc)::value;
    fs->q[o] = 0.0;
    static_for<0, NS>([&](auto i) { fs->zw[o][decltype(i)::value] = 0.0; });
  });

  // the enter part e of a post record: (ex, act, c0, c1) (row, -, fg) (cw0, cw1) (cw2, cw3) (cw4, -); of a fin record: (fg, -)
  auto enter = [&](auto uc, double ab0, double ab1, double ab2, double gv, const rec_i4 (&e)[Q - 1]) {
    constexpr int u = decltype(uc)::value;
    static_for<0, NS>([&](auto vc) { constexpr int v = decltype(vc)::value; if constexpr (v != u) win[tri(u, v)] = 0.0; });
    double diag = 0.0, yv = 0.0;
    double zv[NF > 0 ? NF : 1];
    if constexpr (NF > 0) {
      const int row = e[1].x;
      static_for<0, NF>([&](auto oc) {
        constexpr int o = decltype(oc)::value;
        const double cwo = o % 2 == 0 ? rec_f64(e[2 + o / 2].x, e[2 + o / 2].y) : rec_f64(e[2 + o / 2].z, e[2 + o / 2].w);
        zv[o] = cwo + (row == o ? gv : 0.0);
      });
    }
    if constexpr (POST) {
      static_for<0, NXM>([&](auto sc) { xs[(L::X + decltype(sc)::value * NS + u) * 64] = 0.0; });
      const int ex = e[0].x;
      if (ex != 0) {                                     // the node was an extra: its state moves from LDS into the window
        const int sl = ex - 1;
        if constexpr (NF > 0) static_for<0, NF>([&](auto oc) {
          constexpr int o = decltype(oc)::value;
          zv[o] = xs[(XZ + sl * NF + o) * 64] + zv[o];
          xs[(XZ + sl * NF + o) * 64] = 0.0;
        });
        static_for<0, NS>([&](auto vc) {
          constexpr int v = decltype(vc)::value;
          if constexpr (v != u) win[tri(u, v)] = xs[(L::X + sl * NS + v) * 64];
        });
        diag = xs[(L::XD + sl) * 64]; yv = xs[(L::XY + sl) * 64];
        static_for<0, NXM>([&](auto oc) {
          constexpr int o = decltype(oc)::value;
          if (o != sl) {
            const int a = o > sl ? o : sl, b = o > sl ? sl : o;
            const int idx = L::XX + a * (a - 1) / 2 + b;
            xs[(L::X + o * NS + u) * 64] = xs[idx * 64];
            xs[idx * 64] = 0.0;
          }
        });
        static_for<0, NS>([&](auto vc) { xs[(L::X + sl * NS + decltype(vc)::value) * 64] = 0.0; });
        xs[(L::XD + sl) * 64] = 0.0; xs[(L::XY + sl) * 64] = 0.0;
      }
    }
    win[tri(u, u)] = diag + ab0;
    win[tri(u, (u + NS - 1) % NS)] += ab1;
    win[tri(u, (u + 1) % NS)] += ab2;
    yw[u] = yv + (POST ? rec_f64(e[POST ? 1 : 0].z, e[POST ? 1 : 0].w) : rec_f64(e[0].x, e[0].y));
    if constexpr (NF > 0) static_for<0, NF>([&](auto oc) { fs->zw[decltype(oc)::value][u] = zv[decltype(oc)::value]; });
    if constexpr (POST) {
      for (int c = e[0].z, c1 = e[0].w; c < c1; ++c)     // long-range couplings of this node: to extras (rare; its loads wait in place)
        xs[(L::X + ecp_slot[c] * NS + u) * 64] += io.ld(ecp_off[c]);
    }
  };

  static_for<0, NS>([&](auto uc) {                       // prologue: the first NS nodes enter an empty window
    constexpr int u = decltype(uc)::value;
    if (u < ntot) {
      const rec_i4 a = rec[u * Q];
      rec_i4 e[Q - 1];
      static_for<1, Q>([&](auto i) { e[decltype(i)::value - 1] = rec[u * Q + decltype(i)::value]; });
      enter(uc, io.ldb(a.x), io.ldb(a.y), io.ldb(a.z), NF > 0 ? io.ldb(a.w) : 0.0, e);
    }
  });

  constexpr int RF = (NS % 2 == 0) ? 2 : NS;
  double ab[RF][3], gvr[RF];
  rec_i4 ra[RF], re[RF][Q - 1];
  static_for<0, RF>([&](auto i) {
    constexpr int s = decltype(i)::value;
    ab[s][0] = ab[s][1] = ab[s][2] = 0.0; gvr[s] = 0.0;
    ra[s] = rec[(NS + s) * Q];                           // (beyond the last node: pad records, band_rec_pad)
    static_for<1, Q>([&](auto j) { re[s][decltype(j)::value - 1] = rec_i4{0, 0, 0, 0}; });
  });
  static_for<0, RF>([&](auto i) { rec_settle(ra[decltype(i)::value]); });
  for (int s0 = 0; s0 < npiv + RF; s0 += NS) {
    static_for<0, NS>([&](auto usc) {
      constexpr int us = decltype(usc)::value;
      constexpr int u = (us + NS - RF % NS) % NS;        // window slot of pivot s - RF
      constexpr int rs = us % RF;                        // ring slot (of pivot s - RF and, afterwards, of pivot s)
      const int sidx = s0 + us;
      const int pp = sidx - RF;
      if (pp >= 0 && pp < npiv) {
        const bool more = pp + NS < ntot;
        const double ab0 = ab[rs][0], ab1 = ab[rs][1], ab2 = ab[rs][2];
        const double d = win[tri(u, u)];
        if (!(d > 0.0)) bad = 1;
        double inv = __builtin_amdgcn_rsq(d);
        inv = inv * fma(-0.5 * d * inv, inv, 1.5);
        inv = inv * fma(-0.5 * d * inv, inv, 1.5);
        double l[NS];
        static_for<1, NS>([&](auto sc) { constexpr int s_ = decltype(sc)::value; l[s_] = win[tri((u + s_) % NS, u)] * inv; });
        const double yp = yw[u] * inv;
        double zp[NF > 0 ? NF : 1];
        if constexpr (NF > 0) static_for<0, NF>([&](auto oc) {
          constexpr int o = decltype(oc)::value;
          zp[o] = fs->zw[o][u] * inv;
          fs->q[o] = fma(zp[o], yp, fs->q[o]);
          static_for<1, NS>([&](auto sc) {
            constexpr int s_ = decltype(sc)::value;
            fs->zw[o][(u + s_) % NS] = fma(-l[s_], zp[o], fs->zw[o][(u + s_) % NS]);
          });
        });
        static_for<1, NS>([&](auto sc) {
          constexpr int s_ = decltype(sc)::value;
          yw[(u + s_) % NS] = fma(-l[s_], yp, yw[(u + s_) % NS]);
          static_for<1, s_ + 1>([&](auto tc) {
            constexpr int t = decltype(tc)::value;
            win[tri((u + s_) % NS, (u + t) % NS)] = fma(-l[s_], l[t], win[tri((u + s_) % NS, (u + t) % NS)]);
          });
        });
        if constexpr (POST) {
          const int am = re[rs][0].y;
          if (am != 0) {
            double le[NXM];
            static_for<0, NXM>([&](auto sc) {
              constexpr int sl = decltype(sc)::value;
              le[sl] = 0.0;
              if (am & (1 << sl)) {
                const double v = xs[(L::X + sl * NS + u) * 64] * inv;
                le[sl] = v;
                xs[(L::XY + sl) * 64] = fma(-v, yp, xs[(L::XY + sl) * 64]);
                if constexpr (NF > 0) static_for<0, NF>([&](auto oc) {
                  constexpr int a = (XZ + sl * NF + decltype(oc)::value) * 64;
                  xs[a] = fma(-v, zp[decltype(oc)::value], xs[a]);
                });
                xs[(L::XD + sl) * 64] = fma(-v, v, xs[(L::XD + sl) * 64]);
                static_for<1, NS>([&](auto tc) {
                  constexpr int t = decltype(tc)::value;
                  constexpr int a = (L::X + sl * NS + (u + t) % NS) * 64;
                  xs[a] = fma(-v, l[t], xs[a]);
                });
              }
            });
            static_for<1, NXM>([&](auto ac) {
              constexpr int a = decltype(ac)::value;
              static_for<0, a>([&](auto bc) {
                constexpr int b = decltype(bc)::value;
                xs[L::xx(a, b) * 64] = fma(-le[a], le[b], xs[L::xx(a, b) * 64]);
              });
            });
          }
        }
        if (more) enter(std::integral_constant<int, u>{}, ab0, ab1, ab2, gvr[rs], re[rs]);
        else {
          static_for<0, NS>([&](auto vc) { win[tri(u, decltype(vc)::value)] = 0.0; });      // nobody enters: the slot is empty
          if constexpr (NF > 0) static_for<0, NF>([&](auto oc) { fs->zw[decltype(oc)::value][u] = 0.0; });
        }
      }
      // The node that enters behind pivot s: its values in flight for RF steps.  Requested on EVERY path -- beyond the last node
      // the address part is a neighbour's or a pad record's (offset 0) and nobody uses what comes back -- so that the number of
      // loads in flight is the same whichever way the step went, and the wait at their use is for the older ones only.
      ab[rs][0] = io.ldb(ra[rs].x); ab[rs][1] = io.ldb(ra[rs].y); ab[rs][2] = io.ldb(ra[rs].z);
      if constexpr (NF > 0) gvr[rs] = io.ldb(ra[rs].w);
      // The records.  A wait for one scalar value waits for every scalar load in flight, and the compiler puts it at the value's
      // first use -- the test of `act` at the top of a step, right behind the requests of the step before.  So the wait is taken
      // HERE, once per step, for the records the NEXT step uses (requested a step ago: they have landed), and only then are this
      // step's requests issued: nothing a step reads is still in flight while it runs.
      constexpr int nrs = (us + 1) % RF;
      rec_settle(ra[nrs]);
      static_for<1, Q>([&](auto j) { rec_settle(re[nrs][decltype(j)::value - 1]); });
      int nx = sidx + NS;
      asm volatile("" : "+s"(nx));                       // (the requests stay behind the settled values)
      static_for<1, Q>([&](auto j) { re[rs][decltype(j)::value - 1] = rec[nx * Q + decltype(j)::value]; });      // its enter part
      ra[rs] = rec[(nx + RF) * Q];                       // the address part of the node RF steps behind it
    });
  }
}

template <int NSF, int NSP, int NXM, int NF>
__device__ __forceinline__ void fom_band_fnrec_body(BandDev p, const BandFinRec* __restrict__ fin_rec, const BandPostRec* __restrict__ post_rec,
                                                    const int* __restrict__ ecp_slot, const int* __restrict__ ecp_off,
                                                    const int* __restrict__ schur_off, double* __restrict__ Gw, int64_t S,
                                                    double* __restrict__ qoi, int* __restrict__ info) {
  extern __shared__ __attribute__((aligned(16))) double xlds[];
  const int lane = threadIdx.x;
  const int64_t blk = blockIdx.x;
  double* __restrict__ Gs = Gw + blk * (int64_t)p.gsize * 64;
  Io io{__builtin_amdgcn_make_buffer_rsrc(Gs, 0, p.gsize * 512, 0x00020000), lane * 8};
  double* xs = xlds + lane;
  int bad = 0;
  constexpr int NIFT = (NSF - 1) * NSF / 2;
  {
    double win[NSF * (NSF + 1) / 2], yw[NSF];
    for (int f = 0; f < p.nfins; ++f) {
      const int npiv = p.npf, ntot = p.npf + p.nif;
      band_sweep_rec<NSF, false, NXM, 0>(io, xs, (rec_p)(unsigned long long)(fin_rec + f * ntot), ecp_slot, ecp_off, npiv, ntot, win, yw, bad);
      fin_functional_out<NSF>(p, io, yw, f, npiv, p.nif);
      int k = 0;
      for (int t = 0; t < p.nif; ++t)
        for (int s = 0; s <= t; ++s, ++k) {
          const int a = (npiv + t) % NSF, b = (npiv + s) % NSF;
          double v = 0.0;
          static_for<0, NSF>([&](auto ac) {
            static_for<0, decltype(ac)::value + 1>([&](auto bc) {
              constexpr int ua = decltype(ac)::value, ub = decltype(bc)::value;
              v = ((a == ua && b == ub) || (a == ub && b == ua)) ? win[tri(ua, ub)] : v;
            });
          });
          const int off = schur_off[f * NIFT + k];
          io.st(io.ld(off) + v, off);
        }
    }
  }
  FnState<NF, NSP> fs;
  {
    double win[NSP * (NSP + 1) / 2], yw[NSP];
    band_sweep_rec<NSP, true, NXM, NF>(io, xs, (rec_p)(unsigned long long)post_rec, ecp_slot, ecp_off, p.npost, p.npost, win, yw, bad, &fs);
  }
  const int64_t s = blk * 64 + lane;
  const double nanv = __builtin_nan("");
  if (bad && info != nullptr && s < S) atomicOr(&info[s], 1);
  if (s < S)
    static_for<0, NF>([&](auto oc) {                     // each distinct row once, stored to all its output columns
      constexpr int o = decltype(oc)::value;
      if (o < p.n_obs)
        for (int c = p.out_ptr[o], c1 = p.out_ptr[o + 1]; c < c1; ++c) qoi[s * p.n_out + p.out_col[c]] = bad ? nanv : fs.q[o];
    });
}

// ---- the post's backward sweep with the other waves as loaders ----------------------------------------------------------------
// L^T w = y is a recurrence over the pivots: one wave computes, and what it waits for is the next column of L from HBM (written
// non-temporally by the forward sweep; a register ring of four columns left 0.9 us per pivot at one wave per CU).  The window is
// dead by now, so LDS holds two buffers of CB columns (NS + 1 doubles per lane each: l_1..l_B, 1/L_jj, y_j): while wave 0
// substitutes chunk k out of one, the waves 1 .. WV-1 deposit chunk k - 1 into the other, from registers they requested DL chunk
// steps earlier (HBM latency under load is several steps); one `s_waitcnt lgkmcnt(0); s_barrier` per chunk -- not
// __syncthreads(), whose vmcnt(0) would drain the loaders' pipeline.  The pivot's table entries and its couplings to the extras
// stay with wave 0 (register ring, requested RT pivots ahead, their scalars three more): 1.54 -> 1.09 ms per 16k samples at m = 20.
// What is left is mostly those scalar loads: they share lgkmcnt with the LDS reads, so every wait for an LDS value also waits
// for them; shipping them through LDS as well (complete pivot records built by the loaders) made the LOADERS wait for them
// instead (2.8 ms).
// (columns per chunk: six while two buffers of them fit; four at NS = 26, where the loaders' register sets shrink with it)
constexpr int bsweep_cb(int NS) { return NS > 22 ? 4 : 6; }
template <int NS, int NXM, int WV, int WVI>
__device__ __forceinline__ void band_bsweep_ldsw(const BandDev& p, const Io& io, double* __restrict__ xs, const PostTables& T, int e0,
                                                 int npiv, int L0) {
  constexpr int CB = bsweep_cb(NS), COLS = NS + 1, BUF = CB * COLS, WXO = 2 * BUF;       // LDS (doubles per lane): 2 x CB x (NS + 1) | WX[NXM]
  constexpr int U = NS / gcd_c(NS, CB) * CB;                                   // unroll: window slots and chunk positions compile-time
  constexpr int NP = WV - 1;                                                   // loader waves
  static_assert(WV >= 2 && (2 * BUF + NXM) * 512 <= 160 * 1024, "ring fits LDS (launch_ldsw sizes the allocation)");
  const int kmax = (npiv - 1) / CB;
  auto exchange = [&]() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); };
  constexpr int MINE = WVI > 0 ? (CB - (WVI - 1) + NP - 1) / NP : 0;      // columns of a chunk this loader fetches: i = WVI - 1 + j NP
  constexpr int MA = MINE > 0 ? MINE : 1;
  auto fetch = [&](int k, double (&col)[MA][COLS]) {     // request the own columns of chunk k (nothing is waited for here)
    static_for<0, MINE>([&](auto jc) {
      constexpr int j = decltype(jc)::value, i = WVI - 1 + j * NP;
      const int v = k * CB + i;
      if (k >= 0 && v < npiv) {
        const int base = p.offL + L0 + v * NS;
        static_for<0, NS>([&](auto sc) { constexpr int s_ = decltype(sc)::value; col[j][s_] = io.template ldk<s_>(base); });
        col[j][NS] = io.ld(p.offY + e0 + v);
      }
    });
  };
  auto deposit = [&](int k, int par, const double (&col)[MA][COLS]) {
    static_for<0, MINE>([&](auto jc) {
      constexpr int j = decltype(jc)::value, i = WVI - 1 + j * NP;
      if (k >= 0 && k * CB + i < npiv)
        static_for<0, COLS>([&](auto sc) { constexpr int s_ = decltype(sc)::value; xs[(par * BUF + i * COLS + s_) * 64] = col[j][s_]; });
    });
  };
  if constexpr (WVI == 0) static_for<0, NXM>([&](auto sc) { xs[(WXO + decltype(sc)::value) * 64] = 0.0; });
  if constexpr (WVI > 0) {
    constexpr int DL = NS > 22 ? 3 : 4;
    double cs[DL][MA][COLS];
    static_for<0, DL>([&](auto dc) { constexpr int d = decltype(dc)::value; fetch(kmax - d, cs[d]); });
    deposit(kmax, 0, cs[0]);
    fetch(kmax - DL, cs[0]);
    exchange();
    // step for chunk k: deposit chunk k - 1 (set (kmax - k + 1) % DL), refill that set with chunk k - 1 - DL
    for (int k = kmax; k >= 0; k -= DL) {
      static_for<0, DL>([&](auto dc) {
        constexpr int d = decltype(dc)::value;
        if (k - d >= 0) {
          constexpr int si = (d + 1) % DL;
          deposit(k - d - 1, (kmax - (k - d - 1)) & 1, cs[si]);
          fetch(k - d - 1 - DL, cs[si]);
          exchange();
        }
      });
    }
  } else {
    exchange();                                          // chunk kmax is in buffer 0
    double ww[NS];
    static_for<0, NS>([&](auto i) { ww[decltype(i)::value] = 0.0; });
    // (a pivot takes ~0.6 us here: the couplings are requested RT = 6 pivots ahead, the scalars they depend on three more)
    constexpr int RT = NS > 22 ? 4 : 6;                 // (a divisor of the unroll U where that keeps the code size down)
    double lxv[RT][NXM];
    int am_r[RT], ex_r[RT];
    struct Q { int am, k, ex; };
    // (raw table entries only: any arithmetic on them here would wait for the scalar loads where they are issued)
    auto tables = [&](int q) -> Q { Q r{0, 0, 0}; if (q >= 0 && q < npiv) { r.am = T.act[q]; r.k = T.lx_ptr[q]; r.ex = T.ent_extra[q]; } return r; };
    auto request = [&](auto rc, const Q& t) {             // pivot whose tables are t -> ring slot rc
      constexpr int rs = decltype(rc)::value;
      am_r[rs] = t.am; ex_r[rs] = t.ex;
      if (t.am != 0) {
        int k = p.offLx + t.k;
        static_for<0, NXM>([&](auto sc) { constexpr int sl = decltype(sc)::value; if (t.am & (1 << sl)) { lxv[rs][sl] = io.ld(k); ++k; } });
      }
    };
    constexpr int UT = U / gcd_c(U, RT) * RT;             // (the table ring's slot is compile-time too)
    const int vtop = npiv - 1 + RT;
    Q q1 = tables(vtop - RT), q2 = tables(vtop - RT - 1), q3 = tables(vtop - RT - 2);
    for (int p0 = vtop / UT * UT; p0 >= 0; p0 -= UT) {
      static_for<0, UT>([&](auto rc) {
        constexpr int uu = UT - 1 - decltype(rc)::value;
        constexpr int u = uu % NS, rs = uu % RT, ci = uu % CB;
        const int v = p0 + uu;
        if (v <= vtop) {
          if (v < npiv) {
            const int par = (kmax - v / CB) & 1;
            const double* col = xs + (par * BUF + ci * COLS) * 64;
            double acc = col[NS * 64];
            static_for<1, NS>([&](auto sc) { constexpr int s_ = decltype(sc)::value; acc = fma(-col[(s_ - 1) * 64], ww[(u + s_) % NS], acc); });
            const int am = am_r[rs];
            if (am != 0)
              static_for<0, NXM>([&](auto sc) {
                constexpr int sl = decltype(sc)::value;
                if (am & (1 << sl)) acc = fma(-lxv[rs][sl], xs[(WXO + sl) * 64], acc);
              });
            const double wv = acc * col[(NS - 1) * 64];
            io.st(wv, p.offY + e0 + v);
            ww[u] = wv;
            const int ex = ex_r[rs];
            if (ex != 0) xs[(WXO + ex - 1) * 64] = wv;
            if constexpr (ci == 0) exchange();            // chunk v / CB is done: the loaders have filled the other buffer
          }
          const int nx = v - RT;
          if (nx >= 0 && nx < npiv) request(std::integral_constant<int, rs>{}, q1);
          q1 = q2; q2 = q3; q3 = tables(nx - 3);
        }
      });
    }
  }
}

// WV waves per 64 samples: the eight fins are independent (shared over the waves), the post's forward sweep is band_sweep_ldsr,
// its backward sweep runs on wave 0 with a deeper column ring
template <int NSF, int NSP, int NXM, int WV, bool QO>
__device__ __forceinline__ void fom_band_ldsw_body(const BandDev& p, const int* __restrict__ abmap, const double* __restrict__ Fg,
                                                              const int* __restrict__ act,
                                                              const int* __restrict__ lx_ptr, const int* __restrict__ ent_extra,
                                                              const int* __restrict__ ecp_ptr, const int* __restrict__ ecp_slot,
                                                              const int* __restrict__ ecp_off, const int* __restrict__ schur_off,
                                                              const int* __restrict__ iface_elim, const int* __restrict__ obs_ptr,
                                                              const int* __restrict__ obs_idx, const double* __restrict__ obs_w,
                                                              const int* __restrict__ row_fin,
                                                              double* __restrict__ Gw, int64_t S, double* __restrict__ qoi,
                                                              int* __restrict__ info) {
  extern __shared__ __attribute__((aligned(16))) double xlds[];
  const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t blk = blockIdx.x;
  double* __restrict__ Gs = Gw + blk * (int64_t)p.gsize * 64;
  Io io{__builtin_amdgcn_make_buffer_rsrc(Gs, 0, p.gsize * 512, 0x00020000), lane * 8};
  double* xs = xlds + lane;
  const PostTables T{act, lx_ptr, ent_extra, ecp_ptr, ecp_slot, ecp_off};
  constexpr int FLAG = ldsr_state<NSP, NXM>();                         // behind the forward sweep's buffers
  int bad = 0;
  constexpr int NIFT = (NSF - 1) * NSF / 2;
  long long tk[6];
  tk[0] = wall_clock64();
  {
    double win[NSF * (NSF + 1) / 2], yw[NSF];
    for (int f = wv; f < p.nfins; f += WV) {
      const int npiv = p.npf, ntot = p.npf + p.nif;
      band_sweep<NSF, false, NXM, true, QO>(p, io, xs, Fg, abmap, T, f * ntot, f * npiv, npiv, ntot, f * npiv * NSF, win, yw, bad);
      if constexpr (QO) fin_functional_out<NSF>(p, io, yw, f, npiv, npiv);
      int k = 0;
      for (int t = 0; t < p.nif; ++t)
        for (int s = 0; s <= t; ++s, ++k) {
          const int a = (npiv + t) % NSF, b = (npiv + s) % NSF;
          double v = 0.0;
          static_for<0, NSF>([&](auto ac) {
            static_for<0, decltype(ac)::value + 1>([&](auto bc) {
              constexpr int ua = decltype(ac)::value, ub = decltype(bc)::value;
              v = ((a == ua && b == ub) || (a == ub && b == ua)) ? win[tri(ua, ub)] : v;
            });
          });
          const int off = schur_off[f * NIFT + k];
          io.st(io.ld(off) + v, off);
        }
    }
  }
  __syncthreads();                                       // the fins' Schur complements are in the post's value slots (same CU: same L1)
  tk[1] = wall_clock64();
  {
    int badp = 0;
#define FR_W(I) case I: if constexpr (I < WV) band_sweep_ldsr<NSP, NXM, WV, I>(p, io, xs, Fg, abmap, T, p.post_g0, p.post_e0, p.npost, p.npost, p.post_L0, badp); break;
    switch (wv) { FR_W(0) FR_W(1) FR_W(2) FR_W(3) default: break; }
#undef FR_W
    bad |= badp;
  }
  __syncthreads();                                       // the columns of L, y and the extras' couplings are in the workspace
  tk[2] = wall_clock64();
  {
#define FR_W(I) case I: if constexpr (I < WV) band_bsweep_ldsw<NSP, NXM, WV, I>(p, io, xs, T, p.post_e0, p.npost, p.post_L0); break;
    switch (wv) { FR_W(0) FR_W(1) FR_W(2) FR_W(3) default: break; }
#undef FR_W
  }
  __syncthreads();
  tk[3] = wall_clock64();
  if constexpr (!QO)
    for (int f = wv; f < p.nfins; f += WV)
      band_bsweep<NSF, false, NXM>(p, io, xs, T, iface_elim + f * p.nif, f * p.npf, p.npf, p.npf + p.nif, f * p.npf * NSF, p.offY);
  xs[FLAG * 64] = 0.0;
  __syncthreads();
  if (bad) xs[FLAG * 64] = 1.0;                          // a fin's wave may be the only one that saw its failure
  __syncthreads();
  bad = xs[FLAG * 64] != 0.0;
  tk[4] = wall_clock64();

  const int64_t s = blk * 64 + lane;
  const double nanv = __builtin_nan("");
  if (bad) {
    if constexpr (!QO) for (int i = wv; i < p.n; i += WV) io.st(nanv, p.offY + i);
    if (wv == 0 && info != nullptr && s < S) atomicOr(&info[s], 1);
  }
  // (QO: the fins' functionals were written by whichever wave swept the fin -- before the __syncthreads() above -- and w of
  // the post by wave 0: same CU, same L1)
  for (int o = wv; o < p.n_obs; o += WV) {
    const double q = qoi_row(p, io, obs_ptr, obs_idx, obs_w, row_fin, iface_elim, o, QO);
    if (s < S) qoi[s * p.n_obs + o] = bad ? nanv : q;
  }
  if ((p.on & 2) && s == 0 && wv == 0) {                 // FINROM_BAND_TIMING: 100 MHz ticks per phase (after everybody's QoI)
    __builtin_amdgcn_s_sleep(127);
    for (int i = 0; i < 4 && i < p.n_obs; ++i) qoi[i] = (double)(tk[i + 1] - tk[i]);
  }
}

#define FR_BAND_ARGS BandDev p, const int* __restrict__ abmap, const double* __restrict__ Fg, const int* __restrict__ act,                  \
    const int* __restrict__ lx_ptr, const int* __restrict__ ent_extra, const int* __restrict__ ecp_ptr, const int* __restrict__ ecp_slot,  \
    const int* __restrict__ ecp_off, const int* __restrict__ schur_off, const int* __restrict__ iface_elim, const int* __restrict__ obs_ptr, \
    const int* __restrict__ obs_idx, const double* __restrict__ obs_w, const int* __restrict__ row_fin, double* __restrict__ Gw, int64_t S, \
    double* __restrict__ qoi, int* __restrict__ info
#define FR_BAND_PASS p, abmap, Fg, act, lx_ptr, ent_extra, ecp_ptr, ecp_slot, ecp_off, schur_off, iface_elim, obs_ptr, obs_idx, obs_w, row_fin, Gw, S, qoi, info
template <int NSF, int NSP, int NXM, bool QO>
__global__ __launch_bounds__(64) void fom_band_kernel(FR_BAND_ARGS) { fom_band_body<NSF, NSP, NXM, QO>(FR_BAND_PASS); }
// The same sweep for the half plans of mirror-symmetric operators (bandplan.py, BandPlan(mirror=True)), under a name of its own in
// a kernel trace and with a register budget of its own: the second launch bound is the number of waves per SIMD the compiler has
// to leave room for (3: the 154 registers the (5, 8) window takes uncapped; 4: <= 128; 5: <= 96).  DESIGN 5 has the measurements.
#ifndef FINROM_HALF_WPE
#define FINROM_HALF_WPE 3
#endif
template <int NSF, int NSP, int NXM, bool QO>
__global__ __launch_bounds__(64, FINROM_HALF_WPE) void fom_band_half_kernel(FR_BAND_ARGS) { fom_band_body<NSF, NSP, NXM, QO>(FR_BAND_PASS); }
// The half plan with the post as functionals: 5 x 8 more doubles of right-hand-side windows beside the (5, 8) window, two waves per SIMD
#ifndef FINROM_HALF_FN_WPE
#define FINROM_HALF_FN_WPE 2
#endif
template <int NSF, int NSP, int NXM>
__global__ __launch_bounds__(64, FINROM_HALF_FN_WPE) void fom_band_half_fn_kernel(
    BandDev p, const int* __restrict__ abmap, const double* __restrict__ Fg, const int* __restrict__ act, const int* __restrict__ ent_extra,
    const int* __restrict__ ecp_ptr, const int* __restrict__ ecp_slot, const int* __restrict__ ecp_off, const int* __restrict__ schur_off,
    const double* __restrict__ cw, const int* __restrict__ piv_row, const int* __restrict__ piv_off, double* __restrict__ Gw, int64_t S,
    double* __restrict__ qoi, int* __restrict__ info) {
  fom_band_fn_body<NSF, NSP, NXM, BAND_NF>(p, abmap, Fg, act, ent_extra, ecp_ptr, ecp_slot, ecp_off, schur_off, cw, piv_row, piv_off, Gw, S, qoi, info);
}
// ... and on pivot records (BandFnDev::fin_rec / post_rec; FINROM_FOM_NO_PIVOT_RECORDS=1 keeps the kernel above)
template <int NSF, int NSP, int NXM>
__global__ __launch_bounds__(64, FINROM_HALF_FN_WPE) void fom_band_half_fnrec_kernel(
    BandDev p, const BandFinRec* __restrict__ fin_rec, const BandPostRec* __restrict__ post_rec, const int* __restrict__ ecp_slot,
    const int* __restrict__ ecp_off, const int* __restrict__ schur_off, double* __restrict__ Gw, int64_t S, double* __restrict__ qoi,
    int* __restrict__ info) {
  fom_band_fnrec_body<NSF, NSP, NXM, BAND_NF>(p, fin_rec, post_rec, ecp_slot, ecp_off, schur_off, Gw, S, qoi, info);
}
template <int NSF, int NSP, int NXM, int WV, bool QO>
__global__ __launch_bounds__(64 * WV) void fom_band_ldsw_kernel(FR_BAND_ARGS) { fom_band_ldsw_body<NSF, NSP, NXM, WV, QO>(FR_BAND_PASS); }

// kernel arguments of one launch: the QoI-only form reads the combined table FgQ for Fg and the post-only rows for B_obs
#define FR_BAND_LAUNCH_ARGS(qo) p, p.abmap, (qo) ? p.FgQ : p.Fg, p.act, p.lx_ptr, p.ent_extra, p.ecp_ptr, p.ecp_slot, p.ecp_off, p.schur_off, \
    p.iface_elim, (qo) ? p.qobs_ptr : p.obs_ptr, (qo) ? p.qobs_idx : p.obs_idx, (qo) ? p.qobs_w : p.obs_w, p.row_fin, Gw, S, qoi, info

template <int NSF, int NSP, bool QO, int NXM = 8>
int launch_ldsw(const BandDev& p, double* Gw, int64_t nblk, int64_t S, double* qoi, int* info, hipStream_t st) {
  constexpr int WV = 4;
  static_assert(XL<NSP, NXM>::SIZE <= band_xsize(NSP), "workspace slice of the extras");
  constexpr size_t lds_w = (size_t)(ldsr_state<NSP, NXM>() + 1) * 64 * sizeof(double);      // forward: column / row buffers | extras' state | flag
  constexpr size_t lds_b = (size_t)(2 * bsweep_cb(NSP) * (NSP + 1) + NXM) * 64 * sizeof(double);      // backward: two buffers of CB columns + WX
  constexpr size_t lds = lds_w > lds_b ? lds_w : lds_b;
  static_assert(lds <= 160 * 1024, "LDS window");
  static PerDeviceOnce once;
  if (int rc = once.run([&]() -> int {
        FR_HIP(hipFuncSetAttribute((const void*)fom_band_ldsw_kernel<NSF, NSP, NXM, WV, QO>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        return 0; })) return rc;
  hipLaunchKernelGGL((fom_band_ldsw_kernel<NSF, NSP, NXM, WV, QO>), dim3((unsigned)nblk), dim3(64 * WV), lds, st, FR_BAND_LAUNCH_ARGS(QO));
  FR_HIP(hipGetLastError());
  return 0;
}

template <int NSF, int NSP, bool QO, int NXM = 4, bool HALF = false>
int launch_t(const BandDev& p, double* Gw, int64_t nblk, int64_t S, double* qoi, int* info, hipStream_t st) {
  const size_t lds = (size_t)XL<NSP, NXM>::SIZE * 64 * sizeof(double);
  if constexpr (HALF) hipLaunchKernelGGL((fom_band_half_kernel<NSF, NSP, NXM, QO>), dim3((unsigned)nblk), dim3(64), lds, st, FR_BAND_LAUNCH_ARGS(QO));
  else hipLaunchKernelGGL((fom_band_kernel<NSF, NSP, NXM, QO>), dim3((unsigned)nblk), dim3(64), lds, st, FR_BAND_LAUNCH_ARGS(QO));
  FR_HIP(hipGetLastError());
  return 0;
}

template <int NSF, int NSP, int NXM = 2>
int launch_fn(const BandDev& p, const BandFnDev& fn, double* Gw, int64_t nblk, int64_t S, double* qoi, int* info, hipStream_t st) {
  const size_t lds = (size_t)(XL<NSP, NXM>::SIZE + NXM * BAND_NF) * 64 * sizeof(double);      // the extras' state | their functional values
  if (fn.post_rec != nullptr && fn.fin_rec != nullptr)
    hipLaunchKernelGGL((fom_band_half_fnrec_kernel<NSF, NSP, NXM>), dim3((unsigned)nblk), dim3(64), lds, st, p, fn.fin_rec, fn.post_rec,
                       p.ecp_slot, p.ecp_off, p.schur_off, Gw, S, qoi, info);
  else
  hipLaunchKernelGGL((fom_band_half_fn_kernel<NSF, NSP, NXM>), dim3((unsigned)nblk), dim3(64), lds, st, p, p.abmap, p.FgQ, p.act, p.ent_extra,
                     p.ecp_ptr, p.ecp_slot, p.ecp_off, p.schur_off, fn.cw, fn.piv_row, fn.piv_off, Gw, S, qoi, info);
  FR_HIP(hipGetLastError());
  return 0;
}

}  // namespace

#define FR_W4(A, B, X) if (p.NSF == A && p.NSP == B) return qo ? launch_ldsw<A, B, true, X>(p, Gw, nblk, S, qoi, info, st) : launch_ldsw<A, B, false, X>(p, Gw, nblk, S, qoi, info, st);
#ifdef FINROM_BAND_TU_WIDE
// second translation unit (fom_band_wide.hip includes this file with FINROM_BAND_TU_WIDE defined): the NSP = 26, 30 kernels alone take
// as long to compile as everything else in here
int launch_fom_band_wide(const BandDev& p, double* Gw, int64_t nblk, int64_t S, double* qoi, int* info, hipStream_t st, bool qo) {
  FR_W4(8, 26, 10) FR_W4(9, 30, 12)
  set_error("fom band sweep: unsupported window sizes");
  return FINROM_ERR_UNSUPPORTED;
}
#else
bool band_supported(int NSF, int NSP, int NX) {
  if (NX <= 4 && ((NSF == 3 && NSP == 6) || (NSF == 4 && NSP == 10) || (NSF == 5 && NSP == 14))) return true;      // window in registers
  if (NX <= 2 && ((NSF == 3 && NSP == 4) || (NSF == 4 && NSP == 6) || (NSF == 5 && NSP == 8))) return true;        // ... of the half plans (m = 4, 8, 12)
  if (NX <= 8 && ((NSF == 6 && NSP == 18) || (NSF == 7 && NSP == 22))) return true;                                 // window over four waves
  return (NX <= 10 && NSF == 8 && NSP == 26) || (NX <= 12 && NSF == 9 && NSP == 30);                               // (some of the extras' rows in the workspace)
}

int band_path(const BandDev& p, bool qoi_only) {
  const bool qo = qoi_only && p.qo;
  if (p.NSP <= 14) return qo ? FINROM_FOM_PATH_BAND_REGISTERS_QOI : FINROM_FOM_PATH_BAND_REGISTERS;
  return qo ? FINROM_FOM_PATH_BAND_LDS_4WAVE_QOI : FINROM_FOM_PATH_BAND_LDS_4WAVE;
}

// qoi_only: the caller wants no w; with the plan's QoI-only tables installed (BandDev::qo) the fins then ride as functionals
// fn: the plan is a half plan in the functional form of the post (its workspace layout holds nothing else: the caller passes the
// tables with every launch of such a plan)
int launch_fom_band(const BandDev& p, double* Gw, int64_t nblk, int64_t S, double* qoi, int* info, hipStream_t st, bool qoi_only,
                    const BandFnDev* fn) {
  if (nblk == 0) return 0;
  ScopedKernelTimer t(p.NSP <= 14 ? K_FOM_PATH_BAND_REG : K_FOM_PATH_BAND_LDSW, st);
  const bool qo = qoi_only && p.qo;
  if (fn != nullptr) {
    if (!qo || p.out_ptr == nullptr || p.n_obs > BAND_NF) { set_error("fom band sweep: the functional form serves QoI-only calls of a half plan"); return FINROM_ERR_ARG; }
#define FR_T(A, B) if (p.NSF == A && p.NSP == B) return launch_fn<A, B>(p, *fn, Gw, nblk, S, qoi, info, st);
    FR_T(3, 4) FR_T(4, 6) FR_T(5, 8)
#undef FR_T
    set_error("fom band sweep: unsupported window sizes");
    return FINROM_ERR_UNSUPPORTED;
  }
#define FR_T(A, B) if (p.NSF == A && p.NSP == B) return qo ? launch_t<A, B, true>(p, Gw, nblk, S, qoi, info, st) : launch_t<A, B, false>(p, Gw, nblk, S, qoi, info, st);
  FR_T(3, 6) FR_T(4, 10) FR_T(5, 14)
#undef FR_T
  // the half plans of the same meshes (mirror-symmetric operators, bandplan.py): at most two extras alive
#define FR_T(A, B) if (p.NSF == A && p.NSP == B) return qo ? launch_t<A, B, true, 2, true>(p, Gw, nblk, S, qoi, info, st) : launch_t<A, B, false, 2, true>(p, Gw, nblk, S, qoi, info, st);
  FR_T(3, 4) FR_T(4, 6) FR_T(5, 8)
#undef FR_T
  FR_W4(6, 18, 8) FR_W4(7, 22, 8)
  if (p.NSP >= 26) return launch_fom_band_wide(p, Gw, nblk, S, qoi, info, st, qo);
  set_error("fom band sweep: unsupported window sizes");
  return FINROM_ERR_UNSUPPORTED;
}

#endif
#undef FR_W4

}  // namespace finrom
