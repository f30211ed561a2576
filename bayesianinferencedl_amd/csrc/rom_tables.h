// Host-only tables of the reduced model (rom_tables.hip): what finrom_rom_create / _set_mirror / _set_mirror_short (api_rom.hip)
// need of them.
#pragma once
#include "finrom_core.h"

namespace finrom {

// pattern-uniform k-steps (RomDev::tvu): four rows that share ONE list of theta indices; sorted by term count, descending
struct KStep { std::vector<int> pat; int rows[4]; };
// How the rows that do not fill a k-step of their own pattern are packed.  PACK_CONSECUTIVE: rows that follow each other in pattern
// order share a k-step while the union of their patterns has at most kMaxTerms entries -- every list but the short half list.
// PACK_FEWEST (the half list with dropped rows, finrom_rom_set_mirror, DESIGN 4b''): the leftovers are a tenth to a third of such a
// list, so of three packings -- consecutive, nested (pack_nested), padded (every remainder alone in a k-step of its own pattern) -- the
// one with the fewest k-steps wins, among equals the one with the fewest k-steps that need vector arithmetic in the grouped loop,
// then the one with the fewest multiply-adds, then the earlier in this order.
enum { PACK_CONSECUTIVE = 0, PACK_FEWEST = 1 };
// the grouped tables of one record list (build_grouped_tables; the form itself is described at its definition)
struct GroupedTables { std::vector<double> tvg; std::vector<int> kmg, def; int nkg = 0, n_ext = 0, ext_final = 0, live = 0, fma_ksteps = 0; };

int validate_rom_desc(const finrom_rom_desc* a);
int validate_row_weights(const finrom_rom_desc* a, const double* row_weight);      // every weight of a half descriptor is 1 or 2
int validate_rom_mirror(const finrom_rom_desc* a, int n_full, const int32_t* row_node, const double* row_weight, const int32_t* theta_twin);
std::vector<int> rows_by_term_count(const finrom_rom_desc* a);
std::vector<KStep> uniform_ksteps(const finrom_rom_desc* a, const std::vector<int>& order, int rule = PACK_CONSECUTIVE);
std::vector<KStep> mirror_ksteps(const finrom_rom_desc* a, const double* row_weight, std::vector<int>& kclass);
bool build_grouped_tables(const finrom_rom_desc* a, const std::vector<KStep>& ksteps, int rp, GroupedTables& out,
                          const std::vector<int>* kclass = nullptr, int slot0 = 0, int ext0 = 0, bool scale_free = false);
// FINROM_ROM_SHORT_GROUPED (A/B): the short half list keeps a group per leading parameter.  Read where it is called: the handle
// captures it at creation, the host-only exports ask per call.
bool env_rom_short_grouped();
bool short_scale_free(const finrom_rom_desc* a, bool short_grouped);

}  // namespace finrom
