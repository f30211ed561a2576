/*
 * finrom.h -- C ABI of libfinrom_hip.so: the MI355X (gfx950) implementation of the
 * thermal-fin FOM + ROM forward-solve hot path of sheroze1123/BayesianInferenceDL.
 *
 * The reference has no FFI of its own (pure Python); its boundary is the
 * Python class surface.  Each entry point below names the reference call it replaces
 * (paths relative to the reference repository).  The Python mirror of those classes
 * (bayesianinferencedl_amd/fom/forward_solve.py, rom/averaged_affine_ROM.py, ...) binds
 * these symbols through ctypes (bayesianinferencedl_amd/_ffi.py); see INTEGRATION.md.
 *
 * Conventions
 *  - plain pointers and sizes, no C++ / torch types; all arithmetic is IEEE fp64;
 *  - every function returns 0 on success or a negative finrom_status; it never throws
 *    or aborts; finrom_last_error() gives the thread-local message of the last failure;
 *  - descriptor arrays are HOST pointers, borrowed for the duration of the create call
 *    and copied to the device; the handle owns all device memory it allocates;
 *  - batch arrays (x, theta, qoi, w, ...) are DEVICE pointers, row-major [S x dim],
 *    caller-allocated (finrom_malloc or any other HIP allocator, e.g. a torch tensor);
 *  - `stream` is a hipStream_t passed as void* (NULL = the default stream); calls are
 *    asynchronous on that stream unless stated; a handle is used by one host thread at
 *    a time (the reference classes are not re-entrant either).
 *  - info[s] != 0 marks a failed sample (bit 0, value 1: FOM pivot <= 0 or NaN; bit 1, value 2: ROM pivot);
 *    its outputs are NaN, and no other sample of the batch is touched: every output of every other sample has the bits
 *    the same call returns for the batch without the failed samples (tests/test_gpu_rom_flags.py, tests/test_gpu_fom_flags.py).
 *    A NaN, an infinity or an overflowing entry in a sample's row of theta / x is ordinary data and ends as a flagged sample;
 *    a NaN in a sample's row of `data` (gradients) is not a failed sample: info stays 0, the solve's outputs are those of the
 *    clean data, J and every entry of the gradient are NaN.
 *    The full-order factorisation has no pivoting and flags by the sign of its pivots: an operator that is positive definite
 *    in exact arithmetic but singular to rounding can come back flagged.  Measured with one conductivity, or all, at 1e200 (the
 *    Robin term is then 200 digits below the stiffness): 10 of 26 such samples were flagged with NaN outputs, 16 solved with
 *    info 0 and finite outputs; never anything in between (tests/test_gpu_fom_flags.py).
 *  - what a call does with the info it is given, entry point by entry point:
 *      finrom_fom_solve, finrom_fom_gradient, finrom_fom_solve_rhs     OR bit 0 in; nothing is cleared
 *      finrom_rom_solve, finrom_rom_grad                               OR bit 1 in; nothing is cleared
 *      finrom_solve_pairs                                              ORs bit 0 (FOM half) and bit 1 (ROM half) in; nothing is cleared
 *      finrom_romml_grad                                               OVERWRITES info[s] with 0 or the flag
 *      the finrom_hmc_* steps                                          clear the state's info in front of the model's launches
 *    So the caller zero-initialises info for every entry point of the first three rows (a bit that was set on entry is still
 *    set on return, in a flagged and in a clean row alike), and need not for finrom_romml_grad.  finrom_solve_pairs READS info
 *    behind its two halves where it ran the roomy projection kernel (finrom_rom_last_epilogue): a row whose info is not 0 there
 *    -- from this call or from before it -- gets NaN in qoi_r and err.
 */
#ifndef FINROM_H
#define FINROM_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FINROM_ABI_VERSION 12

typedef enum {
  FINROM_OK = 0,
  FINROM_ERR_ARG = -1,      /* bad argument / inconsistent descriptor */
  FINROM_ERR_HIP = -2,      /* a HIP runtime call failed (message has the hipError name) */
  FINROM_ERR_NOMEM = -3,    /* device allocation failed */
  FINROM_ERR_UNSUPPORTED = -4
} finrom_status;

typedef struct finrom_fom_s* finrom_fom_t;
typedef struct finrom_rom_s* finrom_rom_t;
typedef struct finrom_sampler_s* finrom_sampler_t;
typedef struct finrom_mlp_s* finrom_mlp_t;

int finrom_version(void);
const char* finrom_last_error(void);

/* ---- device plumbing (so that callers need no other HIP binding) -------------------- */
int finrom_device_count(int* count);
int finrom_set_device(int ordinal);
int finrom_malloc(void** dptr, size_t bytes);
int finrom_free(void* dptr);
/* Stream capture (HIP graphs).  Library calls may be captured (hmc.run_chains_device captures a whole HMC proposal around
 * finrom_romml_grad), with two rules the library enforces itself: (1) while a capture is open on any stream the library knows
 * of, it issues no hipFree / hipMalloc / synchronous call -- finrom_free and the *_destroy functions QUEUE their work (the
 * handle is dead for the caller at once) and the next library call that finds no capture open runs the queue; finrom_malloc,
 * the *_create functions, the synchronous copies and any call that would have to grow a handle's workspace fail with
 * FINROM_ERR_UNSUPPORTED instead (run the call once with the same batch size before capturing); (2) a workspace that a captured
 * call used is kept alive until its handle is destroyed, even if a later, larger call replaces it -- a replayed graph never
 * points at freed memory (destroying the handle while its graph is still replayed remains the caller's error).
 * The library learns of a capture from the streams it is handed: every entry point queries its `stream` argument, and
 * finrom_note_stream(stream) tells it about a stream without doing anything else (returns 1 if that stream is capturing, else 0;
 * the Python layer calls it with torch's current stream before it frees or destroys anything from a finaliser, which may run
 * inside somebody's capture).  finrom_free_async(ptr, stream): as finrom_free for a buffer whose last user was a launch on
 * `stream` -- the buffer is parked with an event recorded there and its next owner waits for that event (finrom_free assumes the
 * last user has finished or ran on the default stream).  finrom_deferred_count: queued frees / destructions (tests);
 * finrom_flush_deferred runs the queue if no capture is open and returns what is left. */
int finrom_free_async(void* dptr, void* stream);
int finrom_note_stream(void* stream);
int finrom_deferred_count(void);
int finrom_flush_deferred(void);
int finrom_memcpy_h2d(void* dst, const void* src, size_t bytes, void* stream);
int finrom_memcpy_d2h(void* dst, const void* src, size_t bytes, void* stream);
int finrom_memset(void* dst, int value, size_t bytes, void* stream);
int finrom_stream_sync(void* stream);

/* ---- per-kernel timing with HIP events on the launch stream ------------------------- *
 * When enabled every kernel launch of the library is bracketed by hipEventRecord on its
 * stream; finrom_profile_read synchronises and returns, for kernel slot `slot`
 * (0 <= slot < finrom_profile_slots()), its name, launch count and total milliseconds. */
int finrom_profile_enable(int on);
/* finrom_solve_pairs runs its two halves on two streams (default, 1) or serialised on the caller's
 * stream (0; stand-alone kernel timings).  Same results either way. */
int finrom_set_overlap(int on);
int finrom_profile_reset(void);
int finrom_profile_slots(void);
int finrom_profile_read(int slot, const char** name, int64_t* launches, double* total_ms);

/* ---- FOM: batched sparse SPD solve  A(x) w = F  +  QoI ------------------------------ *
 * Replaces Fin.forward + Fin.qoi_operator   (fom/forward_solve.py:270-291, 408-412),
 * and AffineROMFin.forward + .qoi           (rom/averaged_affine_ROM.py:237-258, 312-320)
 * for S samples at once.  The operator is a sparse-affine map on the entries of the
 * Cholesky factor's pattern:  A_e(x) = asm_c0[e] + sum_t asm_w[t] * x[asm_idx[t]],
 * t in [asm_ptr[e], asm_ptr[e+1]), which covers all three reference operators:
 *   x = nodal field k (xdim = n)       int k_h grad w.grad v dx + Bi int w v ds   fom :160-161
 *   x = 9 / 5 fin conductivities       same, through nine_param_to_function        fom :61-91
 *   x = 9 sub-fin averages             sum_i x_i A_i + Bi M                        rom :154-163
 * The symbolic phase (ordering, pattern of L, elimination schedule) is done once on the
 * host (bayesianinferencedl_amd/symbolic.py); all arrays are in the PERMUTED dof order.
 *
 * The numeric phase is a schedule interpreter: per sample it keeps a value vector
 *   G = [ L entries (nnzL, initially the assembled A_e) | 1/L_ii (n) | y, then w (n) ]
 * and executes two op streams (factorisation + L y = F, then L^T w = y).  A wave (64 samples,
 * lane = sample) fetches the global operands of chunk c+1 (fwd_chunk = 8 or 16 ops) before it executes chunk c,
 * so the host must order/pad the forward stream such that a value stored in chunk c is not loaded
 * before chunk c+2 (both streams; the backward stream runs in its own kernel, 8 ops per chunk); checked at create.  Ops (kind, a, b, d), acc = per-sample accumulator,
 * rc = the LDS row cache (cache_slots entries; holds the row being eliminated and whatever the host left in the other slots):
 *   forward  0 FMA acc -= rc[b]*G[a]   (rc[cache_slots] == -1 and rc[cache_slots+1] == 0 are constants:
 *                  "acc = A_e" is an FMA against the first, padding an FMA against the second with a = -1)
 *            3 LDX x = G[a] | 4 FMAX acc -= x*G[a]   (a row entry that does not fit the LDS cache)
 *            5 FINOFF l = acc*G[a]; G[d] = l; if b >= 0: rc[b] = l; acc = 0
 *            6 FINDIAG t = sqrt(acc); G[d] = t; G[nnzL+b] = inv = 1/t; acc = 0 (acc <= 0 flags the sample)
 *            7 YSET acc = rhs[d] | 8 FINY G[d] = acc*inv; acc = 0
 *            9 XFMA acc += imm[d]*x[b] | 10 CADD acc += imm[d]   (fused affine assembly, xdim <= 16: the stream builds
 *                  A_e = c0_e + sum_t w_t x[idx_t] itself, x sits in LDS, and there is no assembly pre-pass: n_alist = 0)
 *           11 FMALL acc -= rc[b]*rc[d]   (both operands in LDS: the host may allocate the slots of rc as a ring, so that
 *                  the entries of the rows finished just before the current one are still there; slots must have been
 *                  written by an earlier FINOFF.  No global operand, hence no chunk distance to respect.)
 *   backward 0 NOP | 1 WFMA acc -= G[a]*G[b] | 3 WSET acc = G[a] | 5 WFIN G[d] = acc*G[a]
 */
typedef struct {
  int32_t n;               /* dofs */
  int32_t nnzL;            /* entries of L */
  int32_t xdim;            /* length of one parameter vector x */
  int32_t n_obs;           /* rows of the observation operator */
  int32_t nasm;            /* entries of asm_idx / asm_w */
  int32_t n_alist;         /* entries of L that carry a value of A and are assembled by the pre-pass (0: fused stream) */
  int32_t cache_slots;     /* LDS row-cache slots the forward stream assumes (1..126): (cache_slots + 5 [+ xdim for a fused
                              stream]) * 512 B of LDS per wave decide how many interpreter waves share a CU (45 slots -> 7) */
  int32_t fwd_chunk;       /* ops per prefetch chunk of the forward stream: 8 or 16 */
  int32_t nops_fwd;        /* multiple of 2*fwd_chunk, the last 2*fwd_chunk ops are padding */
  int32_t nops_bwd;        /* multiple of 16 (two 8-op chunks), the last 16 ops are NOPs */
  const int32_t* a_list;   /* [n_alist] entry indices, ascending */
  const double*  asm_c0;   /* [nnzL] */
  const int32_t* asm_ptr;  /* [nnzL+1] */
  const int32_t* asm_idx;  /* [nasm] */
  const double*  asm_w;    /* [nasm] */
  const double*  rhs;      /* [n]   load vector F (fom :162-163), permuted */
  const int32_t* fwd_kind; const int32_t* fwd_a; const int32_t* fwd_b; const int32_t* fwd_d;   /* [nops_fwd] each */
  const int32_t* bwd_kind; const int32_t* bwd_a; const int32_t* bwd_b; const int32_t* bwd_d;   /* [nops_bwd] each */
  const int32_t* obs_ptr;  /* [n_obs+1]  CSR of B_obs (fom :215-231) over permuted dofs */
  const int32_t* obs_idx;
  const double*  obs_w;
  const int32_t* perm;     /* [n] permuted -> original dof (to return w in caller order) */
  int32_t n_imm;           /* immediates of the XFMA / CADD ops (0 if the stream has none) */
  const double*  imm;      /* [n_imm] */
} finrom_fom_desc;

int finrom_fom_create(const finrom_fom_desc* desc, finrom_fom_t* out);
void finrom_fom_destroy(finrom_fom_t h);
/* x [S x xdim] -> qoi [S x n_obs], optional w [S x n] (NULL to skip), info [S] (NULL ok) */
int finrom_fom_solve(finrom_fom_t h, const double* x, int64_t S,
                     double* qoi, double* w, int32_t* info, void* stream);

/* ---- FOM adjoint gradient (Fin.gradient, fom/forward_solve.py:293-322) ---------------------- *
 * J = 1/2 |B_obs w - data|^2 and dJ/dx_j = v^T (dA/dx_j) w with the adjoint v = -A^{-1} B_obs^T (B_obs w - data)
 * (A is symmetric: the reference's `_adj_F` is the same operator, so the stored factor is reused through a
 * second op stream).  finrom_fom_set_gradient installs, all over PERMUTED dofs:
 *   res_*    the "solve again" op stream (backward-interpreter op format, value region [nnzL+2n, nnzL+3n)),
 *   bt_*     B_obs^T as CSR by dof  (row i: observation indices and weights),
 *   g_*      for every parameter j the list of (row a, column b, weight dA_ab/dx_j) triples.
 * finrom_fom_gradient: x [S x xdim], data [n_obs] (data_per_sample = 0) or [S x n_obs] ->
 * grad [S x xdim], J [S], optional qoi [S x n_obs]; info as for finrom_fom_solve (bit 0 OR-ed in).
 * A flagged sample (info[s] & 1), on each of the three paths (band adjoint, small-batch kernel, interpreter): every entry of its
 * grad, J and qoi is NaN; every other sample keeps the bits of the batch without it, and the handle's workspace carries nothing
 * over into the next call.  A NaN, +inf or negative conductivity in x is flagged.  x = 1e200 is a positive definite operator with
 * finite entries: such a sample is either solved (info 0, every output finite) or flagged with NaN outputs, never in between --
 * which of the two, rounding in the Schur complements decides. */
typedef struct {
  int32_t nops_res;
  const int32_t* res_kind; const int32_t* res_a; const int32_t* res_b; const int32_t* res_d;
  const int32_t* bt_ptr; const int32_t* bt_obs; const double* bt_w;     /* [n+1], [nnz(B_obs)] */
  const int32_t* g_ptr; const int32_t* g_a; const int32_t* g_b; const double* g_w;   /* [xdim+1], [g_ptr[xdim]] */
} finrom_fom_grad_desc;
int finrom_fom_set_gradient(finrom_fom_t h, const finrom_fom_grad_desc* desc);
int finrom_fom_gradient(finrom_fom_t h, const double* x, const double* data, int32_t data_per_sample, int64_t S,
                        double* grad, double* J, double* qoi, int32_t* info, void* stream);

/* ---- FOM, small batches (the scalar call surface: Fin.forward for ONE conductivity, fom :270-291) --------------- *
 * The interpreter above is a throughput design (lane = sample): a lone wave takes ~12 ms per solve at n = 1597.  For small
 * batches finrom_fom_set_small installs a second, latency-oriented schedule of the same factorisation: one workgroup per
 * sample, lane = ROW of L, rows grouped into dependency levels of the elimination (row i needs the rows of its
 * structure), one barrier per level, the value vector in LDS when it fits (nnzL + 2n doubles <= 152 KiB).  All arrays over
 * PERMUTED dofs; entries of L ordered as for the interpreter streams: row-major, diagonal last in its row.
 *   row_ptr/ent_col         structure of L;  pair_ptr/pair_a/pair_b   L_e = (A_e - sum_q L[pair_a[q]] L[pair_b[q]]) (/ L_jj)
 *   asm_c0/asm_ptr/asm_idx/asm_w   A_e = c0_e + sum_t w_t x[idx_t] per entry (empty range: fill entry)
 *   col_ptr/col_ent/col_row strictly-lower entries of column j (backward substitution)
 *   lev_ptr_f/lev_rows_f, lev_ptr_b/lev_rows_b   rows of each forward / backward level
 * finrom_fom_solve and finrom_fom_gradient then use this schedule whenever S <= small_max. */
typedef struct {
  int32_t small_max;        /* largest batch solved with this schedule */
  int32_t npairs, nasm, nlev_f, nlev_b;
  const int32_t* row_ptr; const int32_t* ent_col;                           /* [n+1], [nnzL] */
  const int32_t* pair_ptr; const int32_t* pair_a; const int32_t* pair_b;    /* [nnzL+1], [npairs] x 2 */
  const double*  asm_c0; const int32_t* asm_ptr; const int32_t* asm_idx; const double* asm_w;   /* [nnzL], [nnzL+1], [nasm] x 2 */
  const int32_t* col_ptr; const int32_t* col_ent; const int32_t* col_row;   /* [n+1], [nnzL-n] x 2 */
  const int32_t* lev_ptr_f; const int32_t* lev_rows_f;                      /* [nlev_f+1], [n] */
  const int32_t* lev_ptr_b; const int32_t* lev_rows_b;                      /* [nlev_b+1], [n] */
} finrom_fom_small_desc;
int finrom_fom_set_small(finrom_fom_t h, const finrom_fom_small_desc* desc);

/* ---- FOM, frontal band sweep (the throughput path of finrom_fom_solve / finrom_solve_pairs) ------------------------ *
 * Same solve as the interpreter (Fin.forward + qoi_operator, fom/forward_solve.py:270-291, 408-412), ordered for the shape
 * of the fin: fin by fin from the tip to the root, then up the post row by row (bayesianinferencedl_amd/bandplan.py).
 * The factorisation then only touches a window of NS = B + 1 consecutive nodes, which the kernel keeps in registers
 * (lane = sample); finished columns of L are written once and read once.  Segment node g (fins: npf own nodes followed by
 * their nif interface nodes; then the post) brings three entries, diagonal, coupling to the previous node, coupling to the
 * node B back: the values of the PHYSICAL slots abmap[3g..3g+2] (slots with the same affine record may be shared; the slots
 * the fins write to must be private); slot value AB[e] = ab_c0[e] + sum_t ab_w[t] x[ab_idx[t]], t in [ab_ptr[e], ab_ptr[e+1])
 * (a pre-pass over the nAB physical slots).  A fin leaves its Schur complement on its interface nodes: entry (t, s), t >= s,
 * is added to the physical slot schur_off[f][..]; ecp_off are physical slots too.
 * Couplings longer than B make the far node an *extra* of the post sweep: act[p] = bit mask of extra slots that pivot p
 * updates (their L values are stored at lx_ptr[p]..), ent_extra[p] = slot + 1 if node p was an extra before it entered the
 * window, (ecp_slot, ecp_off) in [ecp_ptr[p], ecp_ptr[p+1]) = couplings AB[off] of node p to extras, set when p enters.
 * Supported windows: (NSF, NSP) = (3, 6), (4, 10), (5, 14) (m = 4, 8, 12; window in registers), NX <= 4, and (6, 18), (7, 22)
 * (m = 16, 20; the post's window over four waves), NX <= 8, and (8, 26), NX <= 10, (9, 30), NX <= 12 (m = 24, 28; same kernel); otherwise FINROM_ERR_UNSUPPORTED and the handle keeps using the
 * interpreter -- as it does when the load Fg is not zero on the fins' own nodes (the sweep does not carry a fin's load to its
 * interface).  finrom_fom_gradient uses the band layout once finrom_fom_set_band_gradient has installed its tables. */
typedef struct {
  int32_t NSF, NSP, NX;      /* window slots of a fin sweep / of the post sweep, extra slots */
  int32_t nfins, npf, nif;   /* fins, pivots per fin, interface nodes per fin */
  int32_t npost;             /* pivots of the post sweep; n = nfins * npf + npost */
  int32_t nAB, nterms;       /* PHYSICAL value slots, terms of their affine map */
  int32_t nLx;               /* stored extras' L values per sample (= lx_ptr[npost]) */
  const double* ab_c0; const int32_t* ab_ptr; const int32_t* ab_idx; const double* ab_w;   /* [nAB], [nAB+1], [nterms] x 2 */
  const int32_t* abmap;      /* [3 (nfins (npf + nif) + npost)] physical slot of each of the three entries of a segment node */
  const double* Fg;          /* [nfins * (npf + nif) + npost] load per segment node (0 for interface nodes inside a fin) */
  const int32_t* act; const int32_t* lx_ptr; const int32_t* ent_extra;      /* [npost], [npost+1], [npost] */
  const int32_t* ecp_ptr; const int32_t* ecp_slot; const int32_t* ecp_off;  /* [npost+1], [ecp_ptr[npost]] x 2 */
  const int32_t* schur_off;  /* [nfins][nif (nif + 1) / 2] */
  const int32_t* iface_elim; /* [nfins][nif] elimination index of each interface node */
  const int32_t* perm;       /* [n] elimination index -> dof */
  const int32_t* obs_ptr; const int32_t* obs_idx; const double* obs_w;      /* B_obs (CSR) over elimination indices */
  /* Optional (all five or none): the QoI-only form, used when a solve asks for no w (the dataset loop keeps only the
   * observables, generate_fin_dataset.py:93-100).  A fin's own nodes are leaves of the elimination and carry no load, so an
   * observation row's weights on them can ride through the fin's forward sweep as its right-hand side and leave a functional of
   * the fin's interface values; the fin's factor, y and backward sweep are then never stored or run (csrc/fom_band.hip).
   *   qoi_FgQ [as Fg]   the weights of the fin's row on the fin's segment nodes (own, then interface), Fg on the post's;
   *   qoi_row_fin [n_obs]  the fin whose functional belongs to row o, or -1; a fin belongs to at most one row;
   *   qoi_obs_*         CSR of what remains of B_obs: post nodes only, without the row's own fin's interface nodes.
   * Checked on the host against obs_*: both descriptions must be the same operator, entry by entry. */
  const double* qoi_FgQ; const int32_t* qoi_row_fin;
  const int32_t* qoi_obs_ptr; const int32_t* qoi_obs_idx; const double* qoi_obs_w;
} finrom_fom_band_desc;
int finrom_fom_set_band(finrom_fom_t h, const finrom_fom_band_desc* desc);
/* The checks finrom_fom_set_band applies before it touches the device, for a FOM of n dofs, xdim parameters and n_obs
 * observation rows: every index the kernels dereference, no missing table, npf >= NSF and npost >= NSP, and the slots the
 * fins write their Schur complements to (schur_off) private -- not shared between fins, not repeated, read by one entry
 * only (the four-wave kernel sweeps the fins of a sample block on different waves).  Host only: usable without a GPU. */
int finrom_fom_band_validate(const finrom_fom_band_desc* desc, int32_t n, int32_t xdim, int32_t n_obs);

/* The half problem of a MIRROR-SYMMETRIC operator, for the calls that want no w (finrom_fom_solve with w == NULL, the FOM half of
 * finrom_solve_pairs).  Where the conductivity, the load and the observation operator are the same left and right of the fin's
 * symmetry line x = 3 (the five-parameter conductivity on the lattice mesh), so is w, and the sweep only has to solve the left half
 * up to that line: four fins, a post half as wide, under a third of the multiply-adds and of the factor.  `desc` describes the half
 * problem 1/2 E^T A E u = 1/2 E^T F like any band plan (bayesianinferencedl_amd/bandplan.py, BandPlan(mirror=True)): n_half dofs,
 * n_rows DISTINCT observation rows with their QoI-only tables (required: a row and its mirror twin are one row, a self-mirrored row
 * is folded onto the left nodes), windows (3, 4), (4, 6) or (5, 8) with NX <= 2; desc->perm is the identity (no w leaves this plan).
 * Computed row o is stored to the output columns out_col[out_ptr[o] .. out_ptr[o + 1]) of the handle's n_obs -- every column
 * exactly once -- NaN and the info flag of a sample that is not positive definite included.  Calls that want w, gradients and
 * finrom_fom_solve_rhs keep the plan of finrom_fom_set_band, which must have been called; finrom_fom_last_path reports
 * FINROM_FOM_PATH_BAND_REGISTERS_QOI.  FINROM_ERR_UNSUPPORTED when the window sizes are not built in: nothing changes then.
 * Whether an operator table IS symmetric is the caller's finding (engine.py tests c0, every column of W, the load and the rows of
 * B_obs under the mesh's mirror permutation to 1e-13 of each table's largest entry; FINROM_NO_MIRROR=1 at engine creation keeps
 * the full plan for every call). */
int finrom_fom_set_band_mirror(finrom_fom_t h, const finrom_fom_band_desc* desc, int32_t n_half, int32_t n_rows, const int32_t* out_ptr,
                               const int32_t* out_col);
/* Its checks, host only: finrom_fom_band_validate for (n_half, xdim, n_rows), plus the output map for n_obs columns. */
int finrom_fom_band_mirror_validate(const finrom_fom_band_desc* desc, int32_t n_half, int32_t xdim, int32_t n_rows, int32_t n_obs,
                                    const int32_t* out_ptr, const int32_t* out_col);
/* The post as functionals: where the half descriptor fits -- n_rows <= 5, every row's fin weights on the one fin its qoi_row_fin
 * names, no post node an interface node of two fins that rows own -- finrom_fom_set_band_mirror derives, per distinct row o, the
 * weights c_o on the post and lets them ride the post's forward sweep as right-hand sides: q_o = (L^-1 c_o)^T (L^-1 f), no stored
 * factor, no backward sweep; the plan's workspace is then nAB + nfins x nif doubles per sample.  A descriptor that does not fit
 * keeps the stored-factor form, as every descriptor does with FINROM_FOM_POST_STORED=1 in the environment of the set call.
 * finrom_fom_band_mirror_validate checks the derived tables too (every index in range, the operator rebuilt from them equal to
 * obs_*).  finrom_fom_band_mirror_functionals (host only) returns them: *fits = 0 and nothing written, or *fits = 1 and
 * cw [npost x 5] (pivot-major: row o's post-only weight on post pivot t at cw[5 t + o]), piv_row [npost] (the row whose fin has
 * pivot t as an interface node, -1: none) and piv_off [npost] (f * nif + k: that node is interface node k of fin f). */
int finrom_fom_band_mirror_functionals(const finrom_fom_band_desc* desc, int32_t n_half, int32_t xdim, int32_t n_rows, int32_t n_obs,
                                       const int32_t* out_ptr, const int32_t* out_col, int32_t* fits, double* cw, int32_t* piv_row,
                                       int32_t* piv_off);
/* 0: the handle has no half plan; 1: half plan with the post's factor stored; 2: half plan with the post as functionals. */
int finrom_fom_band_mirror_form(finrom_fom_t h);
/* Pivot records of the functional form: what its sweeps read per pivot -- nine tables of the descriptor and the derived ones above --
 * gathered into one fixed-size record per ENTERING node, which the kernel requests with wide scalar loads two steps before it
 * needs them.  Offsets are in BYTES into a sample block's workspace slice (slot << 9: 64 lanes of 8 bytes).
 *   fin record k = f (npf + nif) + t: the three value slots of node t of fin f and qoi_FgQ of that node;
 *   post record t < npost: node t's three value slots; gv = the slot its row's fin left g in (nAB + piv_off[t]) where t is an
 *     interface node of a row's fin (row = piv_row[t] >= 0), else a slot the sweep may load and discard (the node's own first
 *     entry); ent_extra[t], ecp_ptr[t] and [t + 1], qoi_FgQ, cw[5 t ..]; act = act[t - NSP] for t >= NSP, the pivot that
 *     leaves the window as t enters it, 0 before;
 *   post records npost .. npost + NSP - 1: act of the last NSP pivots, behind which nobody enters; everything else zero.
 * finrom_fom_set_band_mirror installs them with the functional form unless FINROM_FOM_NO_PIVOT_RECORDS=1 is in the environment of
 * the set call (the sweep then reads the tables themselves; same results bit for bit).  finrom_fom_solve sweeps on them at every
 * batch size; finrom_solve_pairs where its FOM half runs on the CU-masked stream (batches of 16 384 samples and more beside the
 * one-wave projection), and on the tables otherwise.  The records are checked like every derived
 * table: the source tables rebuilt from them, entry by entry (finrom_fom_band_records_check does the same for records a caller
 * hands in).  finrom_fom_band_mirror_records (host only): *fits as for finrom_fom_band_mirror_functionals; fin_rec takes
 * nfins (npf + nif) records, post_rec npost + NSP. */
typedef struct { int32_t off[3]; int32_t pad0; double fg; double pad1; } finrom_fom_band_fin_rec;                    /* 32 bytes */
typedef struct { int32_t off[3]; int32_t gv; int32_t ex, act, c0, c1; int32_t row, pad0; double fg; double cw[5]; double pad1; } finrom_fom_band_post_rec;   /* 96 bytes */
int finrom_fom_band_mirror_records(const finrom_fom_band_desc* desc, int32_t n_half, int32_t xdim, int32_t n_rows, int32_t n_obs,
                                   const int32_t* out_ptr, const int32_t* out_col, int32_t* fits, finrom_fom_band_fin_rec* fin_rec,
                                   finrom_fom_band_post_rec* post_rec);
/* Host only: 0 if the records are the ones the (validated) descriptor's tables give, FINROM_ERR_ARG and a message naming the
 * field otherwise. */
int finrom_fom_band_records_check(const finrom_fom_band_desc* desc, int32_t n_half, int32_t xdim, int32_t n_rows, int32_t n_obs,
                                  const int32_t* out_ptr, const int32_t* out_col, const finrom_fom_band_fin_rec* fin_rec,
                                  const finrom_fom_band_post_rec* post_rec);
/* 1: the handle's half plan sweeps on pivot records; 0: it reads the tables (or there is no functional form). */
int finrom_fom_band_mirror_records_on(finrom_fom_t h);

/* The adjoint gradient on the band sweep's layout (finrom_fom_gradient for batches beyond the small-batch schedule): after the
 * full sweep the workspace holds the factor and w; A v = -B_obs^T (B_obs w - d) is solved with the stored columns (one forward
 * substitution, one more backward sweep) and grad_j = sum dA_ab/dx_j v_a w_b is contracted there.  Tables over the band plan's
 * ELIMINATION indices (finrom_fom_band_desc::perm):  bt_* = B_obs^T as CSR by elimination index (row e: observation indices and
 * weights);  g_* = for every parameter j the (a, b, dA_ab/dx_j) triples.  Needs finrom_fom_set_band; without it (or for meshes
 * without window sizes) finrom_fom_gradient keeps the interpreter's stored factor (finrom_fom_set_gradient). */
typedef struct {
  const int32_t* bt_ptr; const int32_t* bt_obs; const double* bt_w;     /* [n+1], [nnz(B_obs)] */
  const int32_t* g_ptr; const int32_t* g_a; const int32_t* g_b; const double* g_w;   /* [xdim+1], [g_ptr[xdim]] */
} finrom_fom_band_grad_desc;
int finrom_fom_set_band_gradient(finrom_fom_t h, const finrom_fom_band_grad_desc* desc);

/* General right-hand sides for the operator of each sample: out[s][k][:] = A(x_s)^-1 rhs[s][k][:], k < nrhs, rhs / out [S x nrhs x n]
 * row-major in dof order -- the incremental state and incremental adjoint solves of Fin.hessian_action (fom/forward_solve.py:
 * 344-368: `solve(self._a == rhs)` with a new right-hand side for the same conductivity).  One band sweep factors A(x_s), the
 * columns then stream back once per right-hand side (forward substitution + backward sweep on the stored factor).  Needs
 * finrom_fom_set_band (FINROM_ERR_UNSUPPORTED otherwise); info as for finrom_fom_solve: non-zero for a sample whose operator is not
 * positive definite, and that sample's out is NaN in EVERY entry of every right-hand side (the failed pivot's reciprocal square
 * root is NaN in the stored factor; the forward substitution carries it to the last pivot, the backward sweep from there to every
 * dof).  Lane = sample: no other sample's bits change.
 * Batches whose workspace would exceed 48 GiB run in pieces of whole 64-sample blocks, here, in finrom_fom_solve and in
 * finrom_fom_gradient alike; FINROM_FOM_WORKSPACE_BYTES=<n> (read per call) puts another bound in its place, so that a test can make
 * a small batch run in pieces (64 samples a piece at the least).  The outputs do not depend on the pieces. */
int finrom_fom_solve_rhs(finrom_fom_t h, const double* x, int64_t S, const double* rhs, int32_t nrhs, double* out, int32_t* info,
                         void* stream);

/* ---- which schedule ran (Fin.forward has ONE solver, fom/forward_solve.py:286; this library has several schedules of the
 * same factorisation, picked by batch size and mesh) ------------------------------------------------------------------- *
 * finrom_fom_last_path: the schedule the most recent finrom_fom_solve / finrom_fom_gradient / finrom_solve_pairs call on
 * this handle launched (FINROM_FOM_PATH_NONE before the first call).  Tests assert on it so that a dispatch change cannot
 * silently route a case away from the kernel it was written for; each path also has its own finrom_profile_* slot.
 * finrom_fom_set_small_max moves the batch-size threshold of the small-batch schedule on an existing handle (0 = never;
 * negative = error); it does not install a schedule that finrom_fom_set_small has not installed. */
#define FINROM_FOM_PATH_NONE 0
#define FINROM_FOM_PATH_SMALL_LDS 1        /* fom_small_kernel<true>: one workgroup per sample, value vector in LDS */
#define FINROM_FOM_PATH_SMALL_GLOBAL 2     /* fom_small_kernel<false>: value vector in the workspace */
#define FINROM_FOM_PATH_INTERPRETER 3      /* fom_vm_kernel + fom_bwd_kernel (schedule interpreter) */
#define FINROM_FOM_PATH_BAND_REGISTERS 4   /* fom_band_kernel: frontal band sweep, front in registers (m <= 12) */
#define FINROM_FOM_PATH_BAND_LDS_4WAVE 5   /* fom_band_ldsw_kernel: post's window over four waves + LDS exchange (m = 16 ... 28) */
#define FINROM_FOM_PATH_BAND_LDS_1WAVE 6   /* retired, never returned */
#define FINROM_FOM_PATH_BAND_REGISTERS_QOI 7   /* fom_band_kernel, QoI-only form: fins ride as functionals, no w */
#define FINROM_FOM_PATH_BAND_LDS_4WAVE_QOI 8   /* fom_band_ldsw_kernel, QoI-only form */
int finrom_fom_last_path(finrom_fom_t h);
int finrom_fom_set_small_max(finrom_fom_t h, int32_t small_max);

/* ---- ROM: batched LSPG reduced solve ------------------------------------------------- *
 * Replaces AffineROMFin.forward_nine_param_reduced + .qoi_reduced
 * (rom/averaged_affine_ROM.py:278-310, 323-333):
 *   psi = (sum_p theta_p A_p + Bi M) Phi ; A_r = psi^T psi ; B_r = psi^T F ;
 *   w_r = A_r^{-1} B_r ; qoi_r = (B_obs Phi) w_r.
 * The host passes the row-sparse tables Psi_p = A_p Phi (the reference's precomputed
 * `dA_dsigmak_phi`, :215-220) as one list of r-vectors ("terms"): row j of psi is
 *   sum_{t in [row_ptr[j], row_ptr[j+1])} theta[term_p[t]] * term_val[t][:]
 * with theta[0] == 1 for the constant Robin term and theta[1..P] the parameters.
 */
typedef struct {
  int32_t n;               /* rows of psi (dofs; any order) */
  int32_t r;               /* basis size */
  int32_t P;               /* number of parameters (theta has P entries per sample) */
  int32_t n_obs;
  int32_t nterms;
  const int32_t* row_ptr;  /* [n+1] */
  const int32_t* term_p;   /* [nterms] 0 = constant, 1..P = parameter index + 1 */
  const double*  term_val; /* [nterms x r] row-major */
  const double*  rhs;      /* [n]  F in the same row order */
  const double*  obs_phi;  /* [n_obs x r] B_obs Phi (rom :212) */
} finrom_rom_desc;

int finrom_rom_create(const finrom_rom_desc* desc, finrom_rom_t* out);
void finrom_rom_destroy(finrom_rom_t h);
/* HOST ONLY (no device is touched; for tests of the host logic): the GROUPED k-step tables finrom_rom_create builds for r <= 80
 * (the reference forms psi = A(theta) Phi row by row, rom/averaged_affine_ROM.py:291-297 -- here the rows are
 * sorted by the sub-domain that scales them and accumulated divided by its conductivity).  Sizes first (kmg = tvg = ext_def =
 * NULL), then the tables:  kmg [(nkg + 8) x 8] records {first slot, terms, flags (1: first coefficient is 1, 2: multiply the
 * accumulators by ext[factor] first), factor, ext indices of the <= 4 coefficients};  tvg [n_slots x 4 x rp] table rows
 * (rp = r rounded up to 16);  ext_def [n_ext x 3]: ext[l] = (theta'[a] / theta'[b]) ^ (1 + squared), theta'[0] = 1;
 * ext_final: the factor behind the last k-step.  nkg = 0: no grouped form for this descriptor. */
int finrom_rom_grouped_tables(const finrom_rom_desc* desc, int32_t* nkg, int32_t* n_ext, int32_t* ext_final, int64_t* n_slots,
                              int32_t* kmg, double* tvg, int32_t* ext_def);
/* The HALF form of a mirror-symmetric reduced model (DESIGN.md 4b'; additive, the reference has no counterpart: it contracts all
 * rows of psi for every sample, rom/averaged_affine_ROM.py:291-297).  Where the affine operator commutes with the mesh's mirror
 * permutation for parameters that equal their twins', and the basis is mirror-symmetric up to rounding, psi^T psi is twice the
 * sum over the rows left of the symmetry line plus the sum over the rows on it.  `desc` is a second descriptor in the same
 * format: its rows are those rows (row_node[i]: the handle's row that half row i stands for; row_weight[i]: 2 left of the line,
 * 1 on it), its terms come from the symmetrised basis, and of two parameters that mirror each other (theta_twin [P], 0-based,
 * an involution) only one appears.  finrom_rom_solve and the ROM half of finrom_solve_pairs then walk this list instead of the
 * full one for every sample whose parameters equal their twins' to 1e-13 relative (decided per sample, inside the kernel; any
 * other sample runs exactly what it ran before); B_r, B_obs Phi, gradients, the small-batch kernels and the offline/online form
 * keep the handle's own tables.  Whether the basis is symmetric ENOUGH is the caller's decision (engine.py: RomEngine.set_mirror's
 * gate).  FINROM_ERR_UNSUPPORTED when the handle has no grouped one-wave form (r > 80): nothing changes then. */
int finrom_rom_set_mirror(finrom_rom_t h, const finrom_rom_desc* desc, const int32_t* row_node, const double* row_weight,
                          const int32_t* theta_twin);
/* Its checks, host only (n_full: the rows of the full descriptor): finrom_rom_create's for `desc`, weights 1 or 2 that add up to
 * n_full, no row listed twice, theta_twin an involution, one parameter of a mirror pair at most. */
int finrom_rom_mirror_validate(const finrom_rom_desc* desc, int32_t n_full, const int32_t* row_node, const double* row_weight,
                               const int32_t* theta_twin);
/* HOST ONLY: the half list as finrom_rom_set_mirror builds it, in the format of finrom_rom_grouped_tables (slots and scalars
 * counted from 0 here; on the handle they sit behind the full list's).  Rows of weight 2 and rows of weight 1 never share a
 * k-step; all k-steps of weight 2 come first, and the factor that follows them carries an exact 2: ext_def's third column is
 * a flag word, bit 0 = squared, bit 1 = times two. */
int finrom_rom_mirror_tables(const finrom_rom_desc* desc, const double* row_weight, int32_t* nkg, int32_t* n_ext, int32_t* ext_final,
                             int64_t* n_slots, int32_t* kmg, double* tvg, int32_t* ext_def);
/* The SHORT half list (DESIGN.md 4b''; additive): a THIRD list beside the half list, from a copy of the half descriptor in which a
 * row that is zero up to rounding for every theta has no terms (row_ptr[i + 1] == row_ptr[i]) -- engine.py's
 * RomEngine.mirror_skip_rows selects such rows under the half form's gate, which probes parameters in [theta_lo, theta_hi].  A
 * sample that would walk the half list walks the short one instead when every parameter lies in that range; outside it the rows
 * left out are not covered by the gate (a conductivity contrast of 1e4 moves qoi_r by 1e-6), and the sample keeps the half list.
 * finrom_rom_set_mirror comes first; `desc` has its row count and `row_weight` its weights.  A descriptor with term-less rows packs
 * the rows that do not fill a k-step of their own pattern for the fewest k-steps, among equal counts for the fewest k-steps with
 * vector arithmetic; one without them keeps the packing of every other list (FINROM_ROM_KEEP_ROWS=1, read by engine.py when the
 * handle is created: no short descriptor is made).
 * The counts of what a list multiplies: rows with terms, k-steps before the padding to a multiple of three, k-steps that need a
 * multiply or multiply-add per block.  finrom_rom_mirror_counts: HOST ONLY, for a descriptor (zeros where it has no grouped
 * form); finrom_rom_mirror_info: of a list installed on a handle, which = 0 the half list, 1 the short list, 2 the compact list
 * (zeros: not installed).
 * (finrom_rom_mirror_tables keeps its signature: its nkg is the padded k-step count, these calls give the rest.) */
int finrom_rom_set_mirror_short(finrom_rom_t h, const finrom_rom_desc* desc, const double* row_weight, double theta_lo, double theta_hi);
/* The COMPACT list (DESIGN.md 4b''; additive): a FOURTH list, the short list's rows rotated inside each pattern class.  A_r does not
 * change when the rows of a class -- the unloaded rows that share one list of theta indices -- are replaced by Q times those rows, Q
 * orthogonal; with Q from the singular vectors of the class's stacked tables most rotated rows are zero up to rounding for every
 * theta and get no terms, like the rows the short list leaves out, under the same gate (engine.py: RomEngine.mirror_compact_rows).
 * finrom_rom_compact_rows, HOST ONLY: from a short descriptor and its weights the compact descriptor's term_val [nterms x r] and rhs
 * [n] (row_ptr and term_p stay): every row times sqrt(weight), its load (desc->rhs = weight F) divided by it -- the compact list
 * has no weight classes, the caller passes it with weights of 1 --; per pattern class a one-sided Jacobi SVD of the stacked
 * tables' rows (never the class Gram matrix); a class is rotated only where leaving out its rotated rows below tau x (the largest
 * singular value over all classes, *sigma_max) saves a k-step of four rows, and then holds the rotated rows, largest first, in
 * its row positions.  row_class [n]: the row's class, -1 for loaded and term-less rows; row_sigma [n]: the class's singular
 * values, largest first, in its row positions (rotated or not); row_keep [n]: 0 for a rotated row below the threshold (the
 * caller gives it no terms); Q, optional [n x q_ld]: row i of a rotated class = sum_j Q[i][j] sqrt(w_j) (row of member j),
 * members in ascending row order.
 * finrom_rom_set_mirror_compact: after finrom_rom_set_mirror_short, same checks; the samples that would walk the short list (mirror
 * test passed, every parameter in its [theta_lo, theta_hi]) walk this one instead in a launch that OFFERS it: finrom_solve_pairs
 * for the batches whose sweep it masks by default (S >= 16 384 beside the band sweep, r <= 80; whatever FINROM_FOM_CUS, the stream or
 * the overlap switch then do) -- qoi_r differs from the short list's at rounding level there --, every launch that offers the short
 * list on a handle created under FINROM_ROM_COMPACT=1 (tests), none under FINROM_ROM_NO_COMPACT=1 (A/B).  finrom_rom_solve on a
 * default handle keeps the short list.  The kernels are the short list's, unchanged: the launch hands them the other records. */
int finrom_rom_compact_rows(const finrom_rom_desc* desc, const double* row_weight, double tau, double* term_val, double* rhs,
                            int32_t* row_class, double* row_sigma, int32_t* row_keep, double* Q, int32_t q_ld, double* sigma_max);
int finrom_rom_set_mirror_compact(finrom_rom_t h, const finrom_rom_desc* desc, const double* row_weight);
int finrom_rom_mirror_counts(const finrom_rom_desc* desc, const double* row_weight, int32_t* live_rows, int32_t* ksteps,
                             int32_t* fma_ksteps);
int finrom_rom_mirror_info(finrom_rom_t h, int32_t which, int32_t* live_rows, int32_t* ksteps, int32_t* fma_ksteps);
/* Which list the most recent projection launch of finrom_rom_solve / finrom_solve_pairs on this handle OFFERED its samples
 * (tests assert on it, like finrom_fom_last_path): FINROM_ROM_FORM_HALF = the launch carried the half list and every sample that
 * passed the per-sample mirror test walked it; FINROM_ROM_FORM_FULL = every sample ran the handle's own tables.  finrom_rom_grad
 * never offers the half list: every projection launch of its sets FINROM_ROM_FORM_FULL and FINROM_ROM_EPILOGUE_STANDARD. */
#define FINROM_ROM_FORM_NONE 0
#define FINROM_ROM_FORM_FULL 1
#define FINROM_ROM_FORM_HALF 2
int finrom_rom_last_form(finrom_rom_t h);
/* Which epilogue the most recent projection launch on this handle ran (tests assert on it): FINROM_ROM_EPILOGUE_ROOMY = the
 * 256-register one-wave kernel that finrom_solve_pairs launches beside the FOM's half sweep for QoI-only calls at r <= 80
 * (FINROM_PROJ_NO_ROOMY=1 when the handle is created: never); FINROM_ROM_EPILOGUE_STANDARD = any other kernel.
 * FINROM_ROM_EPILOGUE_ROOMY_SHORT_WAITS = the roomy kernel whose epilogue waits only where an MFMA's result is read by something
 * other than the next MFMA's accumulator input -- same bits as FINROM_ROM_EPILOGUE_ROOMY, which keeps a fixed wait behind every
 * round of dependent MFMAs.  finrom_solve_pairs launches it where the FOM's sweep runs on its CU-masked stream (large batches);
 * when the handle is created, FINROM_PROJ_FIXED_WAITS=1 says never and FINROM_PROJ_SHORT_WAITS=1 at every batch size.
 * FINROM_ROM_EPILOGUE_ROOMY_BLOCK_ROW = the short-waits kernel that scales and eliminates each block row in place with the 4 x 4
 * block steps of its diagonal tile instead of forming that tile's inverse: qoi_r differs from the other two at rounding level, no
 * less accurate.  finrom_solve_pairs launches it for the batches whose sweep it masks by default (whatever then overrides the mask:
 * a call's bits do not depend on where its kernels run), at r in 65 .. 80, on a handle created under neither switch above; FINROM_PROJ_BLOCK_ROW=1 at creation says at every batch size and r <= 80,
 * FINROM_PROJ_NO_BLOCK_ROW=1 never. */
#define FINROM_ROM_EPILOGUE_NONE 0
#define FINROM_ROM_EPILOGUE_STANDARD 1
#define FINROM_ROM_EPILOGUE_ROOMY 2
#define FINROM_ROM_EPILOGUE_ROOMY_SHORT_WAITS 3
#define FINROM_ROM_EPILOGUE_ROOMY_BLOCK_ROW 4
int finrom_rom_last_epilogue(finrom_rom_t h);
/* theta [S x P] -> w_r [S x r] (NULL to skip), qoi_r [S x n_obs], info [S] (NULL ok);
 * optional A_r [S x r x r] and B_r [S x r] (the state the reference keeps in
 * self._A_r / self._B_r for its gradients, :296-297) -- NULL to skip.
 * info: bit 1 (value 2) is OR-ed in for a sample whose A_r cannot be factored; nothing is cleared (see Conventions).
 * A flagged sample, in every form the call dispatches to: every entry of its qoi_r is NaN, and its w_r is not all finite (the
 * guarantee; every form run so far returns no finite entry in it).  What its A_r and B_r hold is not specified.
 * Every other sample keeps, bit for bit, what the batch without the flagged samples returns, and the handle's
 * grow-only scratch carries nothing over: a clean call after a poisoned one returns the bits of the clean call before it.
 * Workspace: the packed A_r and B_r of a piece of the batch stay under 16 GiB; larger batches run in pieces (multiples of four
 * samples), each offsetting theta and every output.  FINROM_ROM_WORKSPACE_BYTES=<n> (read per call) puts another bound in its
 * place, so that a test can make a small batch run in pieces (four samples a piece at the least); finrom_rom_grad and
 * finrom_solve_pairs alike.  The switch is NOT supported by finrom_romml_grad: its one-sample form needs its batch (<= 64 samples)
 * in one piece and returns FINROM_ERR_UNSUPPORTED ("the one-sample form was announced but not taken") when the switch
 * cuts it; leave the switch unset around that entry point.  A piece chooses its kernels by its own size, so a sample's bits are those of a call on the piece
 * alone, not those of the one-piece call.  finrom_rom_solve makes the pieces equal; finrom_rom_grad cuts whole pieces and leaves
 * the rest to the last one. */
int finrom_rom_solve(finrom_rom_t h, const double* theta, int64_t S,
                     double* w_r, double* qoi_r, double* A_r, double* B_r,
                     int32_t* info, void* stream);

/* ---- offline/online form of the reduced operator (opt-in) ------------------------------------------ *
 * psi = A(theta) Phi = sum_p theta_p Psi_p (rom/averaged_affine_ROM.py:282-290; theta_0 = 1 for the Robin term), so
 *   A_r = psi^T psi = sum_{p <= q} theta_p theta_q G_pq,  G_pq = Psi_p^T Psi_q + (p != q ? Psi_q^T Psi_p : 0),
 *   B_r = psi^T F   = sum_p theta_p Psi_p^T F
 * can be assembled from blocks computed once (the reference precomputes Psi_p = A_p Phi, :215-220, and contracts per
 * sample, :291-297).  finrom_rom_set_gram installs the symmetric r x r blocks G_pq, row-major, one per listed pair
 * 0 <= p <= q <= P (0 = constant term; pairs not listed are zero; at most 64 pairs); Psi_p^T F is derived from the
 * descriptor at create.  finrom_rom_set_projection then selects which form finrom_rom_solve / _grad / finrom_solve_pairs
 * use: FINROM_PROJECTION_DIRECT (default: the per-sample psi^T psi contraction on fp64 MFMA, what the reference
 * executes) or FINROM_PROJECTION_GRAM.  Results agree to round-off (tests run both against the same oracle). */
#define FINROM_PROJECTION_DIRECT 0
#define FINROM_PROJECTION_GRAM 1
int finrom_rom_set_gram(finrom_rom_t h, int32_t npairs, const int32_t* pair_p, const int32_t* pair_q,
                        const double* G);
int finrom_rom_set_projection(finrom_rom_t h, int32_t mode);

/* ---- ROM adjoint gradient (AffineROMFin.grad_reduced, rom/averaged_affine_ROM.py:335-356) ---------- *
 * J = 1/2 |data - (B_obs Phi) w_r|^2 and its gradient with respect to the P affine parameters,
 *   g_i = (psi v_r)^T (A_i Phi w_r),   v_r = A_r^{-T} (B_obs Phi)^T (data - (B_obs Phi) w_r),
 * with psi treated as theta-independent exactly as the reference does.  (The reference then maps g to the
 * nodal field through dsigma_dk: dJ_dk = g^T S, a [P x n] product left to the caller.)
 * finrom_rom_set_gradient installs the host-precomputed blocks G_pi = (A_p Phi)^T (A_i Phi), one r x r matrix
 * per listed pair (p in 0..P with 0 = constant term, i in 0..P-1), each stored COLUMN by column.
 * finrom_rom_grad: theta [S x P], data [n_obs] (data_per_sample = 0) or [S x n_obs] (1) ->
 * J [S], g [S x P]; optional w_r [S x r], qoi_r [S x n_obs]; info as for finrom_rom_solve (bit 1 OR-ed in, nothing cleared; pieces
 * and FINROM_ROM_WORKSPACE_BYTES as there).  Any supported r (<= 208).
 * A flagged sample: J and every entry of g and qoi_r are NaN, w_r is not all finite; every other sample keeps its bits -- the
 * fifteen that share a 16-sample MFMA tile of the batched contraction with it included.  A NaN in a sample's data row
 * (data_per_sample = 1) leaves info, qoi_r and w_r as for the clean data and makes J and every entry of g NaN, for that sample
 * alone.  The arrival counters of the small contraction are back at zero behind every call, a poisoned one included. */
int finrom_rom_set_gradient(finrom_rom_t h, int32_t npairs, const int32_t* pair_p, const int32_t* pair_i,
                            const double* G);
int finrom_rom_grad(finrom_rom_t h, const double* theta, const double* data, int32_t data_per_sample,
                    int64_t S, double* J, double* g, double* w_r, double* qoi_r, int32_t* info, void* stream);

/* ---- learned error model + ROM: value and gradient of the ROM+ML misfit -------------------------------------------- *
 * AffineROMFin.grad_romml (rom/averaged_affine_ROM.py:358-396) for S conductivity fields in one call:
 *   e_NN = model(k) (fp32, the reference's Keras res_bn_fc_model, deep_learning/dl_model.py:149-176, batch normalisation in
 *   inference form),  theta = Sop k,  ROM adjoint against data - e_NN  ->  loss = 1/2 |data - (qoi_r + e_NN)|^2  and
 *   grad = (dJ/dtheta)^T Sop  -  (d e_NN / d k)^T (data - (qoi_r + e_NN))     (:376-395)
 * finrom_mlp_create copies the weights (host pointers, fp32, row-major as listed); n_w <= 64, n_out <= 64.
 * finrom_romml_grad: k [S x n] device, data [n_obs] (data_per_sample = 0) or [S x n_obs]; outputs grad [S x n], loss [S],
 * optional qoi_r / e_nn [S x n_obs] (NULL to skip); Sop [P x n] device (the sub-fin averaging operator = dsigma_dk);
 * finrom_rom_set_gradient must have been called on `rom`.  info [S] (optional) is OVERWRITTEN by finrom_romml_grad -- 0, or the
 * flags of finrom_rom_solve -- so the caller need not clear it.  finrom_mlp_predict: e [S x n_out] only (:360). */
typedef struct {
  int32_t n_in, n_w, n_layers, n_out;
  const float* W0; const float* b0;            /* [n_in x n_w], [n_w]                                  y0 = x W0 + b0 */
  const float* scale; const float* shift;      /* [(n_layers + 1) x n_w]  gamma / sqrt(var + eps), beta - mean * scale; last row: head */
  const float* W; const float* b;              /* [n_layers x n_w x n_w], [n_layers x n_w]             y += elu(bn(y)) W_i + b_i */
  const float* Wh; const float* bh;            /* [n_w x n_out], [n_out]                               out = elu(bn(y)) Wh + bh */
} finrom_mlp_desc;
int finrom_mlp_create(const finrom_mlp_desc* desc, finrom_mlp_t* out);
void finrom_mlp_destroy(finrom_mlp_t h);
int finrom_mlp_predict(finrom_mlp_t h, const double* k, int64_t S, double* e, void* stream);
/* Two limits of the device code, for callers and tests (host arithmetic, no device call).  finrom_mlp_stage_reach: the one-sample
 * form of finrom_romml_grad keeps the hidden and head weights in *stage_floats floats of LDS when the returned value -- one past
 * the furthest index its unguarded loops read -- does not exceed that count and n_layers n_w^2 is a multiple of 4 (*staged = 1);
 * other shapes read the weights from memory (*staged = 0).  Either pointer may be NULL; sizes outside finrom_mlp_create's give
 * FINROM_ERR_ARG.  finrom_mlp_forward_max_in: the largest n_in finrom_mlp_predict and the batched form of finrom_romml_grad take
 * (the input is kept in LDS); beyond it they return FINROM_ERR_UNSUPPORTED before any launch. */
int32_t finrom_mlp_stage_reach(int32_t n_layers, int32_t n_w, int32_t n_out, int32_t* staged, int32_t* stage_floats);
int32_t finrom_mlp_forward_max_in(void);
int finrom_romml_grad(finrom_rom_t rom, finrom_mlp_t mlp, const double* Sop, const double* k, const double* data,
                      int32_t data_per_sample, int64_t S, double* grad, double* loss, double* qoi_r, double* e_nn,
                      int32_t* info, void* stream);
/* The network as a model of its own -- the reference's pure deep-learning surrogate (deep_learning/dl_model.py
 * load_surrogate_model, bayesian_inference/estimate_MAP.py MLSolverWrapper): out = NN(k) [S x n_out], loss [S] = 1/2 |data - out|^2,
 * grad [S x n_in] = -(d NN / d k)^T (data - out), network arithmetic in fp32, loss and grad stored as double.  k, data and the
 * outputs are device pointers; data [n_out] (data_per_sample = 0) or [S x n_out].  grad may be NULL (value only); data and loss
 * are NULL together (prediction only); out may be NULL; at least one output is required (FINROM_ERR_ARG otherwise, with a message,
 * before any device call).  S == 0: returns 0, no launch.
 * Two forms (finrom_mlp_last_form: 0 none yet, 1 per-sample, 2 tile).  S < tile_min: one workgroup per sample, two launches
 * (forward; walk back and first layer's transpose); n_in <= finrom_mlp_forward_max_in().  S >= tile_min (default 4096: the measured
 * crossover at n = 1597; finrom_mlp_set_tile_min, >= 1): 64 samples per workgroup, k read once and the first layer and its transpose on the fp32 matrix
 * cores, every (sample, unit) and (sample, input) product one ordered fma chain: a sample's bits depend neither on S nor on its
 * position in the batch nor on its neighbours; no limit on n_in.  In the tile form a row with a non-finite input gets NaN in out,
 * loss and grad, and every other row keeps its bits.  The tile form keeps zero-padded copies of the weights on the handle, made
 * by the first call that takes it: that call, like one that has to grow a workspace, is refused with FINROM_ERR_UNSUPPORTED and
 * a message while a stream capture is open -- run the same call (same handle, same S) once before the capture. */
int finrom_mlp_misfit_grad(finrom_mlp_t h, const double* k, const double* data, int32_t data_per_sample, int64_t S,
                           double* grad, double* loss, double* out, void* stream);
int finrom_mlp_set_tile_min(finrom_mlp_t h, int64_t tile_min);   /* default 4096; >= 1 */
int finrom_mlp_last_form(finrom_mlp_t h);                        /* 0 none yet, 1 per-sample, 2 tile */

/* ---- HMC trajectories on the device (BASELINE configs[4]) ----------------------------------------------------------------------- *
 * PyMC3's sampler calls the reference's value-and-gradient op once per leapfrog step (bayesian_inference/pymc_func_bayes_inverse.py:
 * 92-104 `err_grad_ROMML`, :148-167 `SqErrorOpROMML.perform`; model :186-203: potential = misfit / sigma^2 on a latent Gaussian
 * field) and does the trajectory's arithmetic itself, on the host.  Here a whole proposal is library launches on device-resident
 * chain state, so that it can be captured once in a HIP graph and replayed (bayesianinferencedl_amd/bayesian_inference/hmc.py):
 *   finrom_hmc_begin     momentum of proposal *jt of the uploaded block, H0 = U + |p|^2 / 2, Kq[0] = K, first half step of p;
 *   finrom_hmc_leapfrog  ONE leapfrog step in the four launches of finrom_romml_grad: the position update k <- k + eps p rides in
 *                        front (every kernel that reads the field forms it; Kq[step & 1] -> Kq[(step + 1) & 1]), the value and
 *                        gradient of the ROM + learned-error misfit at the new point are finrom_romml_grad's, and the momentum
 *                        update p <- p - eps c_pri dU, dU = (k - mean) + (c_lik / c_pri) grad (0 for a flagged sample), rides
 *                        behind the gradient; loss [C] and info [C] of the state are overwritten; grad_out [C x n] optional;
 *   finrom_hmc_end       after n_steps steps: last half step back, U(k) = c_lik loss + c_pri |k - mean|^2 / 2 (inf if flagged),
 *                        Metropolis test log u < H0 - H1, state update, accept counters, optional trace row, *jt += 1, *pt += 1.
 * Potential: i.i.d. Gaussian prior N(mean, 1 / c_pri) per node, likelihood scale c_lik = 1 / sigma^2.  (The reference's own prior,
 * a latent Gaussian field k = mean + U^T v with v ~ N(0, I), is finrom_hmc_leapfrog_field below: the same state in whitened
 * coordinates, mean = 0 and c_pri = 1, so that finrom_hmc_begin / _end compute its Hamiltonian unchanged.)  All arrays are DEVICE
 * pointers owned by the caller; C <= 64 chains advance in lockstep (one sample of the batch each); needs finrom_rom_set_gradient,
 * the direct projection, P <= 16 and a basis the one-sample pipeline serves (r <= 96) -- FINROM_ERR_UNSUPPORTED otherwise.
 * finrom_hmc_end / _end_metric reject a chain whose info is not 0, whose potential is NaN or beyond +-1.7e308, or whose kinetic
 * energy is not finite; a rejected chain's K, U and dU keep their bits.  C == 0: finrom_hmc_begin / _end / _begin_metric /
 * _end_metric return 0 and touch nothing, the counters *jt and *pt included. */
typedef struct {
  int64_t C; int32_t n;                 /* chains, nodes of the field */
  double eps, c_lik, c_pri;             /* leapfrog step, 1 / sigma^2, 1 / tau^2 */
  const double* mean;                   /* [C x n] */
  double* K; double* U; double* dU;     /* chain state: position [C x n], potential [C], grad U / c_pri [C x n] */
  double* Kq[2]; double* P; double* dUq; double* H0;   /* trajectory: positions (ping-pong) [C x n] x 2, momentum, grad U / c_pri, H0 [C] */
  const double* P_block; const double* lu_block;       /* draws of a block of B proposals: momenta [B x C x n], log-uniforms [B x C] */
  int64_t* jt; int64_t* pt;             /* device counters: proposal inside the block, proposal of the chain (trace row - 1) */
  int64_t* accept;                      /* [C] accepted proposals */
  double* trace;                        /* [(proposals + 1) x C x n] or NULL */
  double* loss; int32_t* info;          /* [C] value and flags of the last evaluation */
} finrom_hmc_state;
int finrom_hmc_begin(const finrom_hmc_state* st, void* stream);
int finrom_hmc_leapfrog(finrom_rom_t rom, finrom_mlp_t mlp, const double* Sop, const finrom_hmc_state* st, int32_t step,
                        const double* data, int32_t data_per_sample, double* grad_out, double* qoi_r, double* e_nn, void* stream);
int finrom_hmc_end(const finrom_hmc_state* st, int32_t n_steps, void* stream);
/* finrom_hmc_leapfrog in WHITENED coordinates under the latent Gaussian-field prior of the reference's model (pm.gp.Latent(Matern52)
 * .prior, bayesian_inference/pymc_func_bayes_inverse.py:191-201; PyMC3 samples it non-centred): the state's K / Kq / P / dU are
 * v-space, st->mean must be zeros and st->c_pri == 1; `prior` holds the upper factor U of the field's covariance.
 *   field [C x n] (out): field_mean [n] (or NULL) + U^T v' of this step;  grad_field [C x n] (out): the misfit gradient at it.
 * Three pieces in stream order: v' = v + eps p -> field (finrom_sampler_field's kernel, which also writes v' to Kq[(step + 1) & 1]);
 * the value and gradient of finrom_romml_grad at the field (its plain four launches); dUq = v' + c_lik U grad_field (0 for a flagged
 * sample) and p -= eps dUq behind the pullback (finrom_sampler_pullback's kernel).  The workspace lives on `prior`: run one step
 * with the same C before a capture.  Needs the prior's n and the error model's n_in to be st->n (FINROM_ERR_ARG otherwise). */
int finrom_hmc_leapfrog_field(finrom_rom_t rom, finrom_mlp_t mlp, const double* Sop, finrom_sampler_t prior,
                              const double* field_mean, double* field, double* grad_field, const finrom_hmc_state* st,
                              int32_t step, const double* data, int32_t data_per_sample, double* qoi_r, double* e_nn,
                              void* stream);
/* The chains under the OTHER two models of the inverse problem (hmc.py model="fom" | "rom"): the reference's sampler instantiates the
 * full-order operator (bayesian_inference/pymc_func_bayes_inverse.py:174 `SqErrorOpFOM`), the reduced ones are the alternatives
 * beside it (:175-176).  The two halves of a leapfrog step that do not depend on the model are kernels of their own, with the
 * ping-pong convention of finrom_hmc_leapfrog (k = Kq[step & 1], k' = Kq[(step + 1) & 1]); all arithmetic in double, every fused
 * multiply-add written here as fma(a, b, c) = round(a b + c), nothing else contracted:
 *   finrom_hmc_drift  k'[c][i] = fma(eps, P[c][i], k[c][i]).  With A [P x n] row-major (1 <= P <= 16; DEVICE) also
 *                     theta_out[c][p] = theta0[p] + s_p (theta0 [P] or NULL = 0; ONE rounded addition), s_p = sum_i A[p][i] k'[c][i]
 *                     in block_reduce.h's order: thread t = 0 .. 255 chains s = fma(A[p][i], k'[c][i], s) over i = t, t + 256, ...
 *                     from 0; inside each wave of 64 a butterfly (lane l adds lane l ^ off, off = 32, 16, 8, 4, 2, 1); then
 *                     (w0 + w1) + (w2 + w3).  One 256-thread workgroup per chain: a row's bits depend on that row alone.
 *                     A == NULL: the position update alone (theta0, P, theta_out ignored).
 *   finrom_hmc_kick   the gradient at k' is g[c][i] = grad[c][i], or (grad NULL) fma-chained from 0 over p = 0 .. P - 1:
 *                     g = fma(g_theta[c][p], A[p][i], g); exactly one of grad and g_theta is given (A and P with g_theta).
 *                     grad_out[c][i] = g (optional: the field-space gradient, c_lik / c_pri left out).  For a chain with
 *                     info[c] == 0:  d = k'[c][i] - mean[c][i];  dUq = fma(c_lik / c_pri, g, d);  P = fma(-(eps c_pri), dUq, P)
 *                     (both coefficients formed in double first).  For a chain with info[c] != 0: dUq = 0, P untouched.
 *                     Grid (ceil(n / 256), C): one thread per (chain, node); C <= 65535.
 * Neither has a workspace or allocates: legal while the stream is capturing.  Checks before any device call (FINROM_ERR_ARG, with a
 * message): a null state or field of it, step < 0, P outside 1 .. 16 where A is used, a null theta_out with A, both or neither of
 * grad and g_theta, g_theta without A, c_pri == 0 (kick).  C == 0: returns 0, no launch.
 * The fused steps composed from them -- the graph of a proposal stays one linear chain; loss and info of the state are this step's
 * alone (info is cleared by a kernel in front of the model's launches, which flag into it):
 *   finrom_hmc_leapfrog_fom        drift (no A); finrom_fom_gradient's launches at k' (x = the nodal field: fom's xdim must be n)
 *                                  -> st->loss, st->info, gradient into grad_out (or the handle's own buffer: grad_out NULL); kick.
 *   finrom_hmc_leapfrog_field_fom  finrom_hmc_leapfrog_field with finrom_fom_gradient in the place of finrom_romml_grad (c_pri == 1,
 *                                  mean zeros): field kernel with the position update, the FOM at the field, pullback kernel with
 *                                  the momentum update.
 *   finrom_hmc_leapfrog_rom        drift with A into theta [C x P]; finrom_rom_grad's launches at theta -> st->loss, st->info,
 *                                  g_theta [C x P] (theta, g_theta: caller's buffers); kick with (g_theta, A).  The plain reduced
 *                                  model sees the field through theta = Sop k alone, so ONE entry point serves both priors: i.i.d.
 *                                  A = Sop, theta0 NULL; whitened (k = m + U^T v): A = Sop U^T, theta0 = Sop m, mean zeros,
 *                                  c_pri = 1 -- neither n x n triangular product runs in a step, and no field exists.
 * What the model allocates on first use (workspaces that grow with C) it allocates in the first call: run one step with the same C
 * before a capture.  There are no metric forms of these steps; of the model="ml" entry points below the No-U-turn transition alone
 * has one (finrom_hmc_nuts_ml_metric). */
int finrom_hmc_drift(const finrom_hmc_state* st, int32_t step, const double* A, const double* theta0, int32_t P, double* theta_out,
                     void* stream);
int finrom_hmc_kick(const finrom_hmc_state* st, int32_t step, const double* grad, const double* g_theta, const double* A, int32_t P,
                    double* grad_out, void* stream);
int finrom_hmc_leapfrog_fom(finrom_fom_t fom, const finrom_hmc_state* st, int32_t step, const double* data, int32_t data_per_sample,
                            double* grad_out, double* qoi, void* stream);
int finrom_hmc_leapfrog_field_fom(finrom_fom_t fom, finrom_sampler_t prior, const double* field_mean, double* field, double* grad_field,
                                  const finrom_hmc_state* st, int32_t step, const double* data, int32_t data_per_sample, double* qoi,
                                  void* stream);
int finrom_hmc_leapfrog_rom(finrom_rom_t rom, const double* A, const double* theta0, const finrom_hmc_state* st, int32_t step,
                            const double* data, int32_t data_per_sample, double* theta, double* g_theta, double* grad_out,
                            double* qoi_r, void* stream);
/* The chains under the FOURTH model, the pure deep-learning surrogate of finrom_mlp_misfit_grad (hmc.py model="ml", ml_form=): the one
 * model whose chain needs nothing from any other workgroup, so a whole trajectory can run in one launch.  Same ping-pong convention.
 *   finrom_hmc_leapfrog_ml    ONE step as a linear chain of three launches: (1) k' = fma(eps, P, k) and the per-sample forward of
 *                             finrom_mlp_misfit_grad at k' -> st->loss, out [C x n_out] (or the handle's buffer: out NULL), and
 *                             st->info[c] = 1 where loss[c] is not finite, else 0; (2) its per-sample walk back -> the gradient, into
 *                             grad_out [C x n] (or the handle's buffer: grad_out NULL); (3) finrom_hmc_kick's kernel with that
 *                             gradient.  loss and the gradient are the bits finrom_mlp_misfit_grad returns at k' in its per-sample form.
 *   finrom_hmc_trajectory_ml  steps 0 .. n_steps - 1 in ONE launch: C workgroups of 1024 threads, chain c's workgroup alone carries
 *                             its position, momentum and flags from step to step (workgroup barriers only; no flags, spins or atomics
 *                             between workgroups).  On return Kq[n_steps & 1], P, dUq, loss and info hold the bits n_steps calls of
 *                             finrom_hmc_leapfrog_ml leave there, a flagged chain's included (it keeps stepping: position moved, dUq 0,
 *                             P untouched); the other position buffer may hold anything.  n_steps == 0: no launch.
 * Under the latent Gaussian-field prior the field folds into the first layer (W0' = U W0, b0' = b0 + W0^T m: hmc.py,
 * dl_model.whiten_first_layer): the same two entry points with mean zeros and c_pri = 1, no triangular product and no field in a step.
 * Checks before any device call: a null state field, handle or data, step / n_steps < 0, c_pri == 0 (FINROM_ERR_ARG); st->n other than
 * the network's n_in (FINROM_ERR_ARG); n_in > finrom_mlp_forward_max_in() or C > 65535 (FINROM_ERR_UNSUPPORTED).  data [n_out]
 * (data_per_sample = 0) or [C x n_out].  C == 0: returns 0, no launch.  The workspaces (tape and out per chain, the gradient) live on
 * the handle and grow in the first call with that C: that call is refused with FINROM_ERR_UNSUPPORTED and a message while a stream
 * capture is open.  finrom_hmc_begin / _end / _end_stage1 / _end_stage2 around them unchanged: a proposal is 3 launches. */
int finrom_hmc_leapfrog_ml(finrom_mlp_t mlp, const finrom_hmc_state* st, int32_t step, const double* data, int32_t data_per_sample,
                           double* grad_out, double* out, void* stream);
int finrom_hmc_trajectory_ml(finrom_mlp_t mlp, const finrom_hmc_state* st, int32_t n_steps, const double* data, int32_t data_per_sample,
                             void* stream);
/* The No-U-turn sampler for the same chains (hmc.py model="ml" with nuts=Nuts(max_depth); the statement: bayesian_inference/nuts.py
 * transition_iterative): ONE launch is one transition of every chain, one 1024-thread workgroup per chain, followed by the counters'
 * advance.  It replaces finrom_hmc_begin, the steps and finrom_hmc_end.  Multinomial NUTS with the generalised U-turn criterion
 * (Betancourt 2017), identity mass, st->eps the step size (no adaptation):
 *   start      p0 = row jt of P_block (finrom_hmc_draw's), H0 = U + |p0|^2 / 2, both edges the state, rho = p0, W = 1, the candidate
 *              the state itself;
 *   doubling   j = 0 .. max_depth - 1: Philox counter (p lo, p hi, j, 3) under the chain's seed, p = proposal0 + *pt: direction o2 & 1
 *              (1: forward), u_top from (o1 o0); 2^j leapfrog steps from that direction's edge, each finrom_hmc_leapfrog_ml's
 *              arithmetic with full-step momenta: p1/2 = fma(-d h, dU, p), k' = fma(d eps, p1/2, k), dU' = fma(c_lik / c_pri, grad,
 *              k' - mean), p' = fma(-d h, dU', p1/2), h = 0.5 eps c_pri;
 *   leaf m     (1, 2, ... over the transition) dE = U' + |p'|^2 / 2 - H0; flagged, dE not finite or dE > 1000: the sub-tree is
 *              discarded and the transition ends (stop reason 3).  Else w = exp(-dE), W_sub += w, u_m from counter (p lo, p hi, m, 4),
 *              the sub-tree's candidate becomes the leaf when u_m W_sub < w, rho_sub += p'.  U-turns inside the sub-tree by O(depth)
 *              checkpoints (nuts.py): turning discards the sub-tree and ends the transition (2);
 *   adoption   the candidate is replaced when u_top W < W_sub; W += W_sub, rho += rho_sub, the edge moves; the transition ends when
 *              rho . p_left <= 0 or rho . p_right <= 0 (1) or at max_depth (0).
 * Both uniforms are ((o1 o0) >> 11) 2^-53 in [0, 1).  Sums (|p|^2, |k - mean|^2, the U-turn products) in a fixed order: thread t chains
 * fused multiply-adds over i = t, t + 1024, ..., a butterfly inside each of the 16 waves, the wave sums pairwise in index order.
 * On return chain c's K, U, dU and loss hold the draw (loss [C] is the STATE's misfit here: it must hold the start point's on the first
 * call), Kq[0] its position (finrom_hmc_stats_update's cand), accept[c] += moved, trace row *pt + 1 the position, tree [rows x C x 4]
 * row *pt = (depth, leapfrog steps, stop reason, moved) and accept_stat [rows x C] row *pt the mean of min(1, w) over the leaves (a
 * diverged leaf counts 0); then jt and pt advance.  tree and accept_stat may be NULL.  P, dUq, H0, lu_block, Kq[1] and info are not used.
 * Refused before any device call: a null state field, handle, data or seeds, c_pri == 0, proposal0 < 0, max_depth outside 1 .. 10,
 * st->n other than the network's n_in (FINROM_ERR_ARG); n_in > finrom_mlp_forward_max_in() or C > 65535 (FINROM_ERR_UNSUPPORTED).
 * C == 0: returns 0, no launch.  The per-chain workspace (edges, walker, candidates, rho, checkpoints) lives on the handle and grows in
 * the first call with that C: that call is refused with FINROM_ERR_UNSUPPORTED and a message while a stream capture is open. */
int finrom_hmc_nuts_ml(finrom_mlp_t mlp, const finrom_hmc_state* st, const uint64_t* seeds, int64_t proposal0, int32_t max_depth,
                       const double* data, int32_t data_per_sample, int32_t* tree, double* accept_stat, void* stream);
/* The same transition under ANY model (hmc.py model="fom" | "rom" | "romml" with nuts=; the statement: nuts.py LeafMachine, which is
 * transition_iterative cut at the model call): the reference samples with pm.NUTS under the FULL-ORDER operator (bayesian_inference/
 * inference.py:21-57,165-166), whose gradient is many launches of many workgroups, so the tree cannot live in one launch.  Here it is
 * ONE LEAF PER LAUNCH with the tree's bookkeeping in memory, and any model's launches sit between two leaves:
 *   transition = finrom_hmc_nuts_begin;  rounds { clear info; the model's value and gradient at Kq[0] -> st->loss, st->info, grad or
 *                g_theta;  finrom_hmc_nuts_leaf } until no chain is active (at most 2^max_depth - 1 rounds);  finrom_hmc_nuts_end.
 * Layout of all three: one 1024-thread workgroup per chain (finrom_hmc_nuts_end: one thread per (chain, node)); element i of every
 * per-chain array belongs to thread i % 1024; every sum in finrom_hmc_nuts_ml's order (thread t chains fused multiply-adds over
 * i = t, t + 1024, ..., a butterfly inside each of the 16 waves, the wave sums pairwise in index order); every fused multiply-add is
 * written fma(a, b, c) below and nothing else contracts; thread 0 decides and the workgroup follows; no workgroup waits on another.
 * The Philox counters, both uniforms, the stop reasons, the tree row and accept_stat are finrom_hmc_nuts_ml's, word for word; with
 * h = 0.5 eps c_pri, d = +-1 the sub-tree's direction, p = proposal0 + *pt:
 *   finrom_hmc_nuts_begin  p0 = row *jt of P_block; H0 = U + |p0|^2 / 2; both edges (k, p, dU) = (K, p0, dU); rho = p0; W = 1; the sum
 *                          of min(1, w) = 0; j = 0, i = 0, m = 0, depth = 0, moved = 0, reason = 0.  Sub-tree 0's draw: counter
 *                          (p lo, p hi, 0, 3): d from o2 & 1, u_top; W_sub = 0.  The walker stands at d's edge with its first half
 *                          kick made: p1/2 = fma(-d h, dU_edge, p_edge), rho_sub = 0; the first drift k' = fma(d eps, p1/2, k_edge) goes
 *                          to Kq[0]; active[c] = 1.
 *   finrom_hmc_nuts_leaf   for a chain with active[c] == 1 (one with active[c] == 0 is left as it is, to the byte), k' = Kq[0], m += 1:
 *                          g[i] = grad[c][i], or (grad NULL) fma-chained from 0 over q = 0 .. P - 1: g = fma(g_theta[c][q], A[q][i], g);
 *                          info[c] == 0:  dk = k' - mean;  dU' = fma(c_lik / c_pri, g, dk);  p' = fma(-d h, dU', p1/2);
 *                          rho_sub += p';  an even i stores the checkpoint (p', rho_sub) at level popcount(i >> 1);
 *                          U' = fma(c_lik, loss[c], 0.5 c_pri |dk|^2);  dE = (U' + 0.5 |p'|^2) - H0.
 *                          info[c] != 0, dE not finite (a NaN or infinite loss makes it so) or dE > 1000: the transition ends, reason 3.
 *                          Else w = exp(-dE); W_sub += w; the sum of min(1, w) += min(1, w); u_m from counter (p lo, p hi, m, 4); when
 *                          u_m W_sub < w the sub-tree's candidate becomes (k', dU', U', loss[c]).  An odd i tests the checkpoints
 *                          q = popcount(i >> 1) down to that minus (trailing one bits of i) plus 1: rho_s = (rho_sub - rho_q) + p_q,
 *                          turning when rho_s . p_q <= 0 or rho_s . p' <= 0: the transition ends, reason 2.  i += 1.
 *                          At the sub-tree's end (i == 2^j): when u_top W < W_sub the candidate is written into K, dU, U and state_loss
 *                          (the candidate IS the state) and moved = 1; W += W_sub; rho += rho_sub; d's edge = (k', p', dU');
 *                          depth = j + 1; rho . p_left <= 0 or rho . p_right <= 0: ends, reason 1; depth == max_depth: ends, reason 0;
 *                          else j += 1, i = 0, the next sub-tree's draw and walker as in finrom_hmc_nuts_begin.
 *                          Then either the next leaf's p1/2 = fma(-d h, dU', p') and drift k'' = fma(d eps, p1/2, k') into Kq[0], or,
 *                          the transition over, active[c] = 0 and Kq[0] = K: every later round evaluates a point known to be good, and
 *                          finrom_hmc_stats_update finds its cand there (with st->loss of the last round as cand_loss).
 *                          THE START POINT'S EVALUATION is a round too: with Kq[0] = K (finrom_hmc_nuts_begin on a copy of the state
 *                          with eps = 0 leaves k' = fma(0, p1/2, K) = K there, and theta_out with it), the model's launches, and the
 *                          caller's active[c] = 2, the leaf call writes the STATE: dU = fma(c_lik / c_pri, g, K - mean) (0 where
 *                          info[c] != 0), U = fma(c_lik, loss[c], 0.5 c_pri |K - mean|^2) (+inf where info[c] != 0 or not finite),
 *                          state_loss[c] = loss[c], active[c] = 0 -- a leaf's arithmetic, so a chain continued from a draw starts
 *                          from the bits the draw had.  Nothing else is touched.
 *   finrom_hmc_nuts_end    accept[c] += moved; trace row *pt + 1 = K; tree [rows x C x 4] row *pt = (depth, m, reason, moved) and
 *                          accept_stat [rows x C] row *pt = (the sum of min(1, w)) / m.  A chain still active cannot exist after
 *                          2^max_depth - 1 rounds; one that is gets reason -1 and the call still returns 0.  Then *jt += 1, *pt += 1.
 * With A [P x n] (1 <= P <= 16; DEVICE) begin and leaf also write theta_out[c][q] = theta0[q] + s_q (theta0 [P] or NULL = 0; ONE
 * rounded addition), s_q = sum_i A[q][i] Kq[0][c][i] in the order above: finrom_hmc_drift's contract with 1024 threads.  The plain
 * reduced model takes it as its input and returns g_theta; i.i.d. prior: A = Sop; whitened: A = Sop U^T, theta0 = Sop m.
 * The workspace is the CALLER's: finrom_hmc_nuts_ws_bytes(C, n, max_depth) bytes at ws, 8-byte aligned -- 13 + 2 max_depth arrays
 * [C x n] (both edges' k, p, dU; the walker's p', p1/2, dU'; the sub-tree candidate's k, dU; rho; rho_sub; a checkpoint (p, rho_sub)
 * per level), then 8 doubles and 8 int32 per chain.  Nothing allocates: all three are legal while the stream is capturing.  The leaf
 * kernel reads j, i, m and d from the workspace, so a captured round is replayed with no node parameter changed.  P, dUq, H0,
 * lu_block and Kq[1] of the state are not used; st->loss and st->info are the last evaluation's, state_loss [C] is the STATE's misfit
 * (it must hold the start point's before the first transition).
 * Refused before any device call, with a message: a null state, descriptor or field of either (tree and accept_stat may be NULL),
 * c_pri == 0, max_depth outside 1 .. 10, proposal0 < 0, a ws not aligned to 8 bytes, both or neither of grad and g_theta, g_theta
 * without A, P outside 1 .. 16 where A is given, A without theta_out (FINROM_ERR_ARG); C > 65535 (FINROM_ERR_UNSUPPORTED).
 * C == 0: returns 0, no launch, no counter moved.  finrom_hmc_nuts_ws_bytes: FINROM_ERR_ARG (negative) for C < 0, n < 1 or a
 * max_depth outside 1 .. 10. */
typedef struct {
  void* ws;                             /* finrom_hmc_nuts_ws_bytes(C, n, max_depth) bytes, DEVICE */
  const uint64_t* seeds;                /* [C], DEVICE */
  int64_t proposal0;                    /* global index of the proposal *pt == 0 stands for */
  int32_t max_depth;                    /* 1 .. 10 */
  double* state_loss;                   /* [C] the state's misfit */
  int32_t* tree;                        /* [rows x C x 4] or NULL */
  double* accept_stat;                  /* [rows x C] or NULL */
  int32_t* active;                      /* [C] 1 while the chain's transition runs */
} finrom_hmc_nuts_tree;
int64_t finrom_hmc_nuts_ws_bytes(int64_t C, int32_t n, int32_t max_depth);
int finrom_hmc_nuts_begin(const finrom_hmc_state* st, const finrom_hmc_nuts_tree* tr, const double* A, const double* theta0, int32_t P,
                          double* theta_out, void* stream);
int finrom_hmc_nuts_leaf(const finrom_hmc_state* st, const finrom_hmc_nuts_tree* tr, const double* grad, const double* g_theta,
                         const double* A, const double* theta0, int32_t P, double* theta_out, void* stream);
int finrom_hmc_nuts_end(const finrom_hmc_state* st, const finrom_hmc_nuts_tree* tr, void* stream);

/* ---- Laplace-preconditioned HMC: a low-rank metric at the MAP point ------------------------------------------------------------- *
 * The reference's working sampler builds a low-rank Gauss-Newton Hessian of the misfit at the MAP point in prior-whitened
 * coordinates and hands it to NUTS as `scaling` (bayesian_inference/inference.py:102-140,165).  Here that is a handle holding
 *   M = I + V diag(lambda) V^T,   V [n x rho] orthonormal columns, lambda_j > 0, 1 <= rho <= 64,
 * the Gauss-Newton Hessian of the whitened potential misfit / sigma^2 + |v|^2 / 2 (1 / sigma^2 INCLUDED in lambda; the reference's
 * H-tilde leaves it out).  Every map is y = x + sum_j c_j V_j (V_j . x), row-wise, sums in a fixed order (a row's bits depend on
 * that row alone):
 *   FINROM_METRIC_M        c = lambda                       FINROM_METRIC_INV      c = -lambda / (1 + lambda)
 *   FINROM_METRIC_SQRT     c = sqrt(1 + lambda) - 1         FINROM_METRIC_INVSQRT  c = 1 / sqrt(1 + lambda) - 1
 * finrom_metric_create  Vt [rho x n] row-major (the eigenvectors as ROWS) and lam [rho] are HOST arrays, copied; refuses rho outside
 *                       1 .. 64, a lambda that is not finite and > 0, and |Vt Vt^T - I|_max > 1e-10 (FINROM_ERR_ARG, with a message).
 * finrom_metric_apply   x, y [S x n] device (y != x), quad [S] device or NULL: quad[s] = x_s . y_s.  One launch, no workspace.
 * finrom_metric_destroy queued while a stream capture is open, like every handle's.
 * Chains under the metric (hmc.py metric=, whitened coordinates under the latent Gaussian-field prior): momenta p ~ N(0, M),
 * kinetic energy p^T M^-1 p / 2, position update eps M^-1 p.
 *   finrom_hmc_begin_metric           finrom_hmc_begin with P_block holding STANDARD normals xi (the same random stream):
 *                                     p = M^(1/2) xi, H0 = U + |xi|^2 / 2 (= U + p^T M^-1 p / 2);
 *   finrom_hmc_leapfrog_field_metric  vel [C x n] (caller's buffer) = M^-1 p, then finrom_hmc_leapfrog_field with vel in the place
 *                                     of p in the position update; gradient, pullback and momentum update (of p) unchanged: one
 *                                     launch more per step, no fork;
 *   finrom_hmc_end_metric             finrom_hmc_end with kinetic energy (|p|^2 - sum_j d_j (V_j . p)^2) / 2, d = lambda / (1 + lambda).
 * None of them allocates: they may be captured once the plain step has run with the same C. */
typedef struct finrom_metric_s* finrom_metric_t;
enum { FINROM_METRIC_M = 0, FINROM_METRIC_INV = 1, FINROM_METRIC_SQRT = 2, FINROM_METRIC_INVSQRT = 3 };
int finrom_metric_create(const double* Vt, const double* lam, int32_t n, int32_t rho, finrom_metric_t* out);
void finrom_metric_destroy(finrom_metric_t h);
int finrom_metric_apply(finrom_metric_t h, int32_t op, const double* x, int64_t S, double* y, double* quad, void* stream);
int finrom_hmc_begin_metric(const finrom_hmc_state* st, finrom_metric_t metric, void* stream);
int finrom_hmc_leapfrog_field_metric(finrom_rom_t rom, finrom_mlp_t mlp, const double* Sop, finrom_sampler_t prior,
                                     const double* field_mean, double* field, double* grad_field, const finrom_hmc_state* st,
                                     int32_t step, const double* data, int32_t data_per_sample, double* qoi_r, double* e_nn,
                                     finrom_metric_t metric, double* vel, void* stream);
int finrom_hmc_end_metric(const finrom_hmc_state* st, finrom_metric_t metric, int32_t n_steps, void* stream);
/* finrom_hmc_nuts_ml under the metric: the reference's sampler as it is called, pm.NUTS(scaling=G_INV, max_treedepth=7)
 * (bayesian_inference/inference.py:102-140,165-166); hmc.py nuts=Nuts(max_depth, metric=...), the statement nuts.py's
 * transition_iterative(metric=).  The same launch, workgroup layout, Philox words, stop reasons, tree row, accept_stat and candidate
 * rule; with the velocity v(x) = M^-1 x = x + sum_j a_j V_j, a_j = c_inv[j] (V_j . x), c_inv = -lambda / (1 + lambda):
 *   start      row jt of P_block holds STANDARD normals xi (finrom_hmc_draw's, unchanged): p0 = M^(1/2) xi, v0 = v(p0),
 *              H0 = U + p0 . v0 / 2, both edges (k, p0, v0, dU), rho = p0;
 *   leaf       p1/2 = fma(-d h, dU, p), k' = fma(d eps, v(p1/2), k), dU' as there, p' = fma(-d h, dU', p1/2), v' = v(p'),
 *              dE = U' + p' . v' / 2 - H0; rho_sub += p';
 *   U-turns    the generalised criterion with p# = M^-1 p (Betancourt 2017, A.4.2): checkpoints hold (p, v, rho_sub),
 *              rho_s = (rho_sub - rho_ckpt) + p_ckpt, turning when rho_s . v_ckpt <= 0 or rho_s . v' <= 0; the tree when
 *              rho . v_left <= 0 or rho . v_right <= 0.
 * Sums of the maps: wave w of the 16 forms V_j . x for j = w, w + 16, w + 32, w + 48 alone (lane l chains fused multiply-adds over
 * elements l, l + 64, ..., a butterfly inside the wave), then y = x + sum_j a_j V_j with j ascending, one fused multiply-add per term
 * (finrom_metric_apply's orders for 16 waves); p' . v' and the U-turn products in finrom_hmc_nuts_ml's order.
 * Refused before any launch: everything finrom_hmc_nuts_ml refuses; a null metric handle, a metric whose n is not st->n
 * (FINROM_ERR_ARG); an n_in that leaves no LDS for the sums, above finrom_mlp_forward_max_in() - 256 (FINROM_ERR_UNSUPPORTED).
 * C == 0: returns 0, no launch.  The workspace is finrom_hmc_nuts_ml's with the velocities' arrays behind it, on the same handle: the
 * first call with a new C is refused with FINROM_ERR_UNSUPPORTED and a message while a stream capture is open. */
int finrom_hmc_nuts_ml_metric(finrom_mlp_t mlp, const finrom_hmc_state* st, finrom_metric_t metric, const uint64_t* seeds,
                              int64_t proposal0, int32_t max_depth, const double* data, int32_t data_per_sample, int32_t* tree,
                              double* accept_stat, void* stream);
/* The step-size warm-up of the No-U-turn chains (hmc.py nuts=Nuts(max_depth, adapt=StepAdapt(target_accept, tune)); the statement
 * nuts.py StepAdapt): dual averaging (Hoffman & Gelman 2014, Algorithm 5) on the accept_stat every transition writes, the reference's
 * `tune=100, target_accept=0.98` (bayesian_inference/inference.py:145,165-166).  Every chain adapts its OWN step, eps [C] on the device.
 *   finrom_hmc_nuts_ml_adapt, finrom_hmc_nuts_ml_metric_adapt, finrom_hmc_nuts_begin_adapt, finrom_hmc_nuts_leaf_adapt
 *       the entry point without _adapt with chain c's step read from eps[c] (DEVICE) in the place of st->eps: one uniform load at
 *       the top of the kernel, h = 0.5 eps[c] c_pri formed where it is formed from st->eps.  With eps[c] == st->eps for every c they
 *       leave the bytes of their counterparts; a chain's bits depend on its own step alone.  (The start point's round of the
 *       leaf-per-round form is finrom_hmc_nuts_begin on a state with eps = 0, and finrom_hmc_nuts_end serves both.)  They refuse
 *       what their counterparts refuse, and a null eps (FINROM_ERR_ARG).
 *   finrom_hmc_step_adapt_update
 *       ONE launch, one thread per chain, behind a transition of either form (after the counters' advance): the transition is row
 *       r = *pt - 1 of accept_stat [rows x C] with global index p = proposal0 + r.  step_size [rows x C] (or NULL) row r = eps, the
 *       step that transition took; then with t = p + 1, a = accept_stat[r][c], ONLY WHILE t <= tune:
 *         w = 1 / (t + t0);  hbar = (1 - w) hbar + w (target - a);  s = sqrt(t);  x = mu - hbar s / gamma;  eta = 1 / (s sqrt(s));
 *         xbar = eta x + (1 - eta) xbar;  eps = exp(x) if t < tune, exp(xbar) if t == tune
 *       every operation as written, one rounding each, nothing contracted: hbar and xbar are the statement's bits, eps is within
 *       the two exponentials' error bounds.  t > tune (tune = 0 included): nothing but step_size is written.  p and a are read from
 *       the device, so a captured launch is replayed with no node parameter changed; nothing allocates: legal while a capture is
 *       open.  The entry point knows no row count: the CALLER sizes accept_stat and step_size to at least *pt rows (the rows the
 *       transitions' own tree and accept_stat arrays need), and a *pt of 0 -- no transition yet -- writes nothing.  Refused before any device call, with a message (FINROM_ERR_ARG): a null descriptor or eps, hbar, xbar; tune < 0; a
 *       target outside (0, 1); gamma or t0 not > 0; C < 0; proposal0 < 0; a null pt or accept_stat.  C == 0: returns 0, no launch. */
typedef struct {
  double* eps; double* hbar; double* xbar;      /* [C] DEVICE: the step of the next transition; the log-domain state */
  double mu, target, gamma, t0;                 /* log(10 eps0); target_accept; 0.05; 10 */
  int64_t tune;                                 /* transitions that adapt: those with global index < tune */
} finrom_hmc_step_adapt;
int finrom_hmc_nuts_ml_adapt(finrom_mlp_t mlp, const finrom_hmc_state* st, const double* eps, const uint64_t* seeds, int64_t proposal0,
                             int32_t max_depth, const double* data, int32_t data_per_sample, int32_t* tree, double* accept_stat,
                             void* stream);
int finrom_hmc_nuts_ml_metric_adapt(finrom_mlp_t mlp, const finrom_hmc_state* st, finrom_metric_t metric, const double* eps,
                                    const uint64_t* seeds, int64_t proposal0, int32_t max_depth, const double* data,
                                    int32_t data_per_sample, int32_t* tree, double* accept_stat, void* stream);
int finrom_hmc_nuts_begin_adapt(const finrom_hmc_state* st, const finrom_hmc_nuts_tree* tr, const double* eps, const double* A,
                                const double* theta0, int32_t P, double* theta_out, void* stream);
int finrom_hmc_nuts_leaf_adapt(const finrom_hmc_state* st, const finrom_hmc_nuts_tree* tr, const double* eps, const double* grad,
                               const double* g_theta, const double* A, const double* theta0, int32_t P, double* theta_out,
                               void* stream);
int finrom_hmc_step_adapt_update(const finrom_hmc_step_adapt* ad, int64_t C, int64_t proposal0, const int64_t* pt,
                                 const double* accept_stat, double* step_size, void* stream);
/* The draws of a block of B proposals ON THE DEVICE (hmc.py rng="philox"), in the layout finrom_hmc_begin / _begin_metric read: row
 * j * C + c of P_block [B x C x n] and of lu_block [B x C] belongs to proposal first_proposal + j of the chain with seed seeds[c]
 * (seeds [C]: DEVICE array).  For seed s and global proposal index p, Philox4x32-10 with key (s lo, s hi):
 *   momentum     counter (p lo, p hi, pair index jb, 0): words (o1 o0) and (o3 o2) give 53-bit uniforms u1 in (0, 1], u2 in [0, 1),
 *                Box-Muller makes xi[2 jb], xi[2 jb + 1] -- row 0 of finrom_sampler_draw_seeded's xi for (seed s, sample p, S = 1);
 *                standard normals also under a metric (finrom_hmc_begin_metric forms p = M^(1/2) xi);
 *   log-uniform  counter (p lo, p hi, 0, 1): a = (o1 << 32) | o0, u = ((a >> 11) + 1) 2^-53 in (0, 1], lu = log u, finite and <= 0.
 * A draw depends on (s, p) and on nothing else: the same chain for any block size B, any deal of the chains over ranks, and for a
 * run continued from its end state with first_proposal = the proposals already made.  One launch on `stream`, one thread per
 * Box-Muller pair, no allocation: legal while the stream is capturing.  Checks before any device call (FINROM_ERR_ARG, with a
 * message): C, B or first_proposal negative, n < 1, a null pointer with B x C > 0.  B == 0 or C == 0: returns 0, no launch. */
int finrom_hmc_draw(const uint64_t* seeds, int64_t C, int32_t n, int64_t first_proposal, int64_t B, double* P_block, double* lu_block,
                    void* stream);
/* The chains' posterior summaries accumulated ON THE DEVICE (hmc.py stats=): one launch behind finrom_hmc_end / _end_metric (or the
 * caller's own state update), grid (ceil(n / 256), C), one thread per (chain, node), no workspace and no allocation: legal while
 * the stream is capturing.  What the reference's drivers take from a kept trace after the run (bayesian_inference/inference.py:
 * 175-214: np.mean / np.std of the trace, the misfit per draw), without the trace.  With q = *pt >= 1 the proposals done in this
 * call (this one included) and g = proposal0 + q - 1 the proposal's global index:
 *   accepted   chain c was accepted iff accept[c] != acc_prev[(q - 1) & 1][c]; the chain's first workgroup alone writes accept[c]
 *              into slot q & 1 (the caller fills slot 0 with the counters before the first proposal);
 *   state      accepted: cur[c, :] = cand[c, :], cur_loss[c] = cand_loss[c];  misfit[q, c] = cur_loss[c], accepted[q, c] = the flag;
 *   draws      g >= burn: t = g - burn + 1, x = cur[c, i]:
 *                d = x - mean;  mean = mean + d / t;  m2 = m2 + d * (x - mean);  bsum = bsum + x;
 *                t % batch == 0:  b = t / batch, bm = bsum / batch,
 *                                 d = bm - bm_mean;  bm_mean = bm_mean + d / b;  bm_m2 = bm_m2 + d * (bm - bm_mean);  bsum = 0.
 * No fused multiply-add, IEEE division, t and b converted exactly: the sums are the bits of hmc.ChainStats.update (NumPy), whatever
 * the cut into blocks, graph or stream order, or the point at which a run was interrupted and continued (everything is indexed
 * by g; the caller hands the sums of the first run to the second).  The statistics are of FIELDS: under the latent Gaussian-field
 * prior `cand` is the step's field buffer, not the whitened state (the variance of a field needs Cov(v) in full).
 * Checks before any device call (FINROM_ERR_ARG, with a message): C, burn or proposal0 negative, n < 1, batch < 1, C > 65535, a
 * null pointer other than misfit / accepted with C > 0.  C == 0: returns 0, no launch. */
typedef struct {
  int64_t C; int32_t n;
  int64_t proposal0;            /* global index of this call's first proposal */
  int64_t burn, batch;          /* draws are the states after proposals with global index >= burn; batch length >= 1 */
  const int64_t* pt;            /* the chain state's counter, already advanced by finrom_hmc_end */
  const int64_t* accept;        /* [C] the chain state's accept counters */
  const double* cand;           /* [C x n] FIELD at the end point of the proposal just tested */
  const double* cand_loss;      /* [C] misfit there */
  double* cur; double* cur_loss;/* [C x n], [C]: field and misfit of the CURRENT state (caller fills them for the start point) */
  int64_t* acc_prev;            /* [2 x C] ping-pong copy of accept */
  double *mean, *m2, *bsum, *bm_mean, *bm_m2;   /* [C x n] each */
  double* misfit; int32_t* accepted;            /* [(proposals + 1) x C] or NULL; row 0 is the start */
} finrom_hmc_stats;
int finrom_hmc_stats_update(const finrom_hmc_stats* s, void* stream);
/* Delayed acceptance (hmc.py correct=; Christen & Fox 2005): the trajectory runs under a surrogate (the reduced model, with or
 * without the learned error), the full-order model decides.  finrom_hmc_end is split into a decision and a commit, and ONE
 * full-order forward solve at the end point (finrom_fom_solve without w) goes in between:
 *   finrom_hmc_end_stage1  finrom_hmc_end's arithmetic up to the decision, through the same device function: the half step back,
 *                          the two sums, Uq[c] = fma(c_lik, loss, 0.5 c_pri dd) (+inf where info != 0, NaN or beyond +-1.7e308),
 *                          ok1[c] = lu_block[*jt C + c] < H0[c] - H1.  Writes ok1 [C] and Uq [C] and NOTHING else: K, U, dU,
 *                          accept, trace and the counters are untouched.  Launch shape, argument checks and the C == 0 rule
 *                          of finrom_hmc_end; ok1 and Uq must not be NULL when C > 0.
 *   finrom_hmc_end_stage2  one 256-thread workgroup per chain; no fused multiply-add but the one written here.  Thread 0, with
 *                          d = data (+ c n_obs when data_per_sample), jt = *st->jt, pt = *st->pt, in this order:
 *                            s = 0;  for o = 0 .. n_obs - 1:  r = qoi_f[c][o] - d[o];  s = fma(r, r, s);   lossF = 0.5 s;
 *                            Dq = c_lik (lossF - st->loss[c]);
 *                            good = info_f[c] == 0 && |lossF| <= 1.7e308 && Dq is finite;
 *                            ok = ok1[c] != 0 && good && lu2_block[jt C + c] < D[c] - Dq;
 *                            cand_loss_f[c] = good ? lossF : NaN;
 *                            correction[(pt + 1) C + c] = good ? Dq : NaN            (where correction is given);
 *                            accept1[c] += ok1[c] != 0;   st->accept[c] += ok;
 *                            ok:  st->U[c] = Uq[c];  D[c] = Dq;  loss_f[c] = lossF.
 *                          Behind a barrier all threads run finrom_hmc_end's commit: K = Kq[n_steps & 1] and dU = dUq where ok,
 *                          the trace row pt + 1 (the new state) where st->trace is given; then *jt += 1, *pt += 1 as there.
 *                          A rejected chain keeps every bit of K, U, dU, D and loss_f.  The weight is w = exp(-D), D = c_lik
 *                          (loss_FOM - loss_surrogate): the priors cancel, and with stage 1 reversible for the surrogate's
 *                          posterior the two stages are reversible for the full-order one.
 * Neither allocates: both are legal while the stream is capturing.  Checks before any device call (FINROM_ERR_ARG, with a
 * message): those of finrom_hmc_end; a null descriptor; n_obs < 1; a null pointer other than correction with C > 0.  C == 0:
 * returns 0 and touches nothing, the counters included. */
typedef struct {
  int32_t n_obs; int32_t data_per_sample;
  const int32_t* ok1; const double* Uq;        /* [C] what finrom_hmc_end_stage1 wrote */
  const double* qoi_f; const int32_t* info_f;  /* [C x n_obs], [C]: finrom_fom_solve at the end point's field */
  const double* data;                          /* [n_obs], or [C x n_obs] with data_per_sample */
  const double* lu2_block;                     /* [B x C] second log-uniforms (finrom_hmc_draw_stage2), row *st->jt */
  double* D; double* loss_f; int64_t* accept1; /* [C] each, the chain's state: correction and full-order misfit of the current
                                                  point (caller fills them for the start point), proposals past stage 1 */
  double* cand_loss_f;                         /* [C] out: the end point's full-order misfit (NaN where flagged) */
  double* correction;                          /* [(proposals + 1) x C] out or NULL; row 0 is the start's D (the caller's) */
} finrom_hmc_da;
int finrom_hmc_end_stage1(const finrom_hmc_state* st, int32_t n_steps, int32_t* ok1, double* Uq, void* stream);
int finrom_hmc_end_stage2(const finrom_hmc_state* st, int32_t n_steps, const finrom_hmc_da* da, void* stream);
/* The second log-uniform of a block of B proposals, for stage 2: lu2_block [B x C], row j * C + c for proposal first_proposal + j of
 * the chain with seed seeds[c] (DEVICE array).  Philox4x32-10, key (s lo, s hi), counter (p lo, p hi, 0, 2), and the conversion
 * of finrom_hmc_draw's log-uniform: a = (o1 << 32) | o0, u = ((a >> 11) + 1) 2^-53, lu2 = log u, finite and <= 0.  It depends on
 * (s, p) alone.  One launch, no allocation.  Checks (FINROM_ERR_ARG, with a message): C, B or first_proposal negative, a null
 * pointer with B x C > 0.  B == 0 or C == 0: returns 0, no launch. */
int finrom_hmc_draw_stage2(const uint64_t* seeds, int64_t C, int64_t first_proposal, int64_t B, double* lu2_block, void* stream);

/* ---- batched multi-start MAP estimation: a projected L-BFGS on the device ------------------------------------------------------- *
 * The reference minimises 0.5 |y(k) - d|^2 + reg(k) with SciPy's L-BFGS-B, one start after another (bayesian_inference/
 * estimate_MAP.py:246-281).  Here S starts advance in lockstep on device-resident state, and a ROUND is three pieces in stream
 * order, the same launches every round (so it can be captured once in a HIP graph and replayed; bayesian_inference/lbfgs.py):
 *   finrom_lbfgs_propose  per running start: the free set, the two-loop L-BFGS direction and the trial point xt = P(x + alpha d)
 *                         (or the next backtracked trial on the stored direction); a stopped start copies x to xt;
 *   (the caller's model)  f_in [S], g_in [S x d] -- or [S x gdim] when G is set -- and info [S] (non-zero: flagged) at xt;
 *   finrom_lbfgs_accept   the pieces the library owns -- g = G^T g_in (G [gdim x d], gdim <= 16) and the Tikhonov term
 *                         0.5 gamma x^T K1 x with gradient gamma K1 x (K1 as CSR) -- then the Armijo test, the backtrack, the
 *                         history ring (m pairs), the stopping tests (SciPy's), the counters and an optional fhist row.
 * finrom_lbfgs_begin projects x (set by the caller to the starts) into [lo, hi], copies it to xt and marks every start running;
 * the first accept after it takes the model's values at x0.  Algorithm: lbfgs.py (minimize_host is its NumPy statement; a
 * projected L-BFGS with Armijo backtracking on the projection arc, not Byrd et al.'s L-BFGS-B).  Every sum has a fixed order:
 * results are the same bits run to run, and a start's result depends on its own row only.
 * status [S]: -1 running, 0 converged (projected gradient or relative reduction), 1 iteration / evaluation limit, 2 line search
 * failed with an empty history, 3 the start itself is flagged or not finite.  A point counts as flagged when info is non-zero, when
 * its value (with the Tikhonov term) is NaN or +-inf, or when any component of its gradient g (after G^T and the Tikhonov term) is:
 * at x0 that is status 3, later a rejected trial.  All arrays are DEVICE pointers owned by the caller;
 * lo / hi [d] or NULL (unbounded side); the caller checks lo <= hi.  work holds FINROM_LBFGS_WORK_DOUBLES(S, d, m) doubles
 * (per start: the s and y rings, the direction, s^T y, y^T y and 8 scalars; the reason of a start's stop is scalar 5:
 * 0 projected gradient, 1 relative reduction, 2 iterations, 3 evaluations, 4 line search, 5 flagged).  fhist [fhist_rows x S]
 * or NULL: row i = f after iteration i.  Tikhonov is on when k1_ptr is set (k1_ptr [d + 1], k1_idx, k1_val).
 * Checks before any device call: S >= 1, d >= 1, 1 <= m <= 16, the required pointers, 1 <= gdim <= 16 when G is set (0
 * otherwise), maxls >= 1 -- FINROM_ERR_ARG with a message naming the argument; d > 4352 is FINROM_ERR_UNSUPPORTED.  No
 * allocation: the calls may be captured. */
#define FINROM_LBFGS_WORK_DOUBLES(S, d, m) ((int64_t)(S) * ((2 * (int64_t)(m) + 1) * (int64_t)(d) + 2 * (int64_t)(m) + 8))
typedef struct {
  int64_t S; int32_t d, m;              /* starts, variables, history pairs */
  double ftol, gtol;                    /* SciPy's: relative reduction, projected-gradient infinity norm */
  int64_t maxiter, maxfun; int32_t maxls;
  const double* lo; const double* hi;   /* [d] or NULL */
  double* x; double* f; double* g; double* xt;   /* [S x d], [S], [S x d], [S x d] (trial point: the model's input) */
  double* work;                         /* FINROM_LBFGS_WORK_DOUBLES(S, d, m) */
  int32_t* status; int64_t* nit; int64_t* nfev;  /* [S] */
  double* fhist; int64_t fhist_rows;    /* [fhist_rows x S] or NULL */
  const double* G; int32_t gdim;        /* [gdim x d] or NULL (then gdim = 0) */
  double gamma; const int32_t* k1_ptr; const int32_t* k1_idx; const double* k1_val;   /* Tikhonov, or k1_ptr = NULL */
} finrom_lbfgs_state;
int finrom_lbfgs_begin(const finrom_lbfgs_state* st, void* stream);
int finrom_lbfgs_propose(const finrom_lbfgs_state* st, void* stream);
int finrom_lbfgs_accept(const finrom_lbfgs_state* st, const double* f_in, const double* g_in, const int32_t* info, void* stream);

/* ---- sub-fin averages  theta = S k  (fom :466-480, rom :404-418) -------------------- *
 * Sop is the dense [P x n] averaging operator on the device (finrom_malloc + h2d). */
int finrom_subfin_avg(const double* Sop, int32_t P, int32_t n,
                      const double* k, int64_t S, double* theta, void* stream);

/* ---- Gaussian-field sampler  k = exp(0.5 * U^T xi) ----------------------------------- *
 * (deep_learning/generate_fin_dataset.py:87-88 with U = make_cov_chol(...),
 *  bayesian_inference/gaussian_field.py:9-31; U is the UPPER factor, row-major [n x n],
 *  host pointer copied at create; anything below the diagonal is an error).  xi [S x n] -> k [S x n]. */
int finrom_sampler_create(const double* U, int32_t n, finrom_sampler_t* out);
void finrom_sampler_destroy(finrom_sampler_t h);
int finrom_sampler_draw(finrom_sampler_t h, const double* xi, int64_t S, double* k, void* stream);
/* The same with xi drawn ON THE DEVICE (the reference draws np.random.randn per sample, generate_fin_dataset.py:87):
 * Philox4x32-10, counter = (global sample index, pair index), key = seed, Box-Muller; sample first_global_sample + s of
 * the stream `seed` is the same numbers whatever shard or GPU draws it.  k [S x n]; xi_out [S x n] or NULL. */
int finrom_sampler_draw_seeded(finrom_sampler_t h, uint64_t seed, int64_t first_global_sample, int64_t S, double* k,
                               double* xi_out, void* stream);
/* The latent Gaussian field's two triangular products with the same factor (HMC under the reference's prior, hmc.py), any S:
 *   finrom_sampler_field     k = mean + U^T v   (mean [n] device or NULL; v, k [S x n] device) -- the map of finrom_sampler_draw
 *                            without the exp;
 *   finrom_sampler_pullback  out = U g          (g, out [S x n] device) -- the gradient of a field-space function pulled back to v.
 * Deterministic: every output is summed in an order set by n alone, and row s does not depend on the other rows of the batch
 * (a chain alone and the same chain in a batch are bit-identical).  Partial sums live in a workspace on the handle, grown outside
 * a stream capture only; calls on one handle must be ordered (one stream, or events). */
int finrom_sampler_field(finrom_sampler_t h, const double* mean, const double* v, int64_t S, double* k, void* stream);
int finrom_sampler_pullback(finrom_sampler_t h, const double* g, int64_t S, double* out, void* stream);

/* ---- the dataset-loop body for S samples in one call ---------------------------------- *
 * (deep_learning/generate_fin_dataset.py:93-100):  FOM solve + QoI on the caller's stream;
 * concurrently, on a stream owned by the library, theta = Sop x (sub-fin averages of the
 * field, or of the interpolated per-fin conductivities) and the LSPG reduced solve + QoI;
 * then err = qoi - qoi_r.  (Large batches of the r <= 80 / m <= 12 pairing: the FOM's band
 * sweep runs on a library stream restricted to three CUs of every shader engine, one
 * where the half plan of finrom_fom_set_band_mirror serves the call -- the
 * HBM-bound sweep then shares fewer SIMDs with the projection, DESIGN.md 5 -- its pack +
 * assembly pre-pass on an unmasked stream, and when the caller's stream is a non-blocking
 * one the ROM half stays on it: no cross-stream wait on the call's critical path.
 * FINROM_FOM_CUS=0 keeps the FOM half on the caller's stream.)
 * The two halves are independent and are joined with HIP events
 * on the caller's stream (every output is ready in stream order behind the call),
 * so the HBM-bound sparse solve overlaps the MFMA-bound projection.
 * Sop: device [P x xdim] (P = the ROM's parameter count, xdim = the FOM's).  Optional
 * outputs (NULL to skip): w [S x n], w_r [S x r], theta [S x P], err [S x n_obs].
 * info [S] must be zero-initialised by the caller: bit 0 (FOM half) and bit 1 (ROM half) are OR-ed in, nothing is cleared, and
 * behind the roomy projection kernel a row whose info is not 0 -- set by this call or before it -- gets NaN in qoi_r and err. */
int finrom_solve_pairs(finrom_fom_t fom, finrom_rom_t rom, const double* Sop,
                       const double* x, int64_t S,
                       double* qoi, double* qoi_r, double* err,
                       double* w, double* w_r, double* theta, int32_t* info, void* stream);

/* ---- the gather at the end for callers without torch.distributed ------------------------------------------------ *
 * The path shards by samples with no data-path collective; the one exchange is an all-gather of per-sample rows (QoI pairs,
 * 144 B per sample) when every rank has finished its shard -- the reference's loop (deep_learning/generate_fin_dataset.py:83-100)
 * run per rank, results collected once.  RCCL over xGMI, loaded with dlopen at the first call (no link-time dependency; a process
 * that already holds PyTorch's RCCL shares it).  Protocol: rank 0 calls finrom_comm_unique_id and hands the FINROM_COMM_ID_BYTES
 * bytes to the other ranks by whatever channel the launcher offers (file, socket, MPI, environment); every rank, with ITS device
 * current (finrom_set_device), calls finrom_comm_init; finrom_gather(send [count], recv [nranks x count]) is an all-gather of
 * `count` doubles per rank on DEVICE buffers, asynchronous on `stream`, rank r's block at recv + r * count.
 * One process per GPU (RCCL rejects two ranks on one device).  bench.py and bayesianinferencedl_amd/distributed.py keep using
 * torch.distributed when torch is the launcher; both routes end in ncclAllGather. */
#define FINROM_COMM_ID_BYTES 128
typedef struct finrom_comm_s* finrom_comm_t;
int finrom_comm_unique_id(void* id_out);
int finrom_comm_init(finrom_comm_t* out, int32_t rank, int32_t nranks, const void* id);
int finrom_gather(finrom_comm_t comm, const double* send, int64_t count, double* recv, void* stream);
int finrom_comm_destroy(finrom_comm_t comm);

/* ---- elementwise helper: err = qoi - qoi_r (generate_fin_dataset.py:99) -------------- */
int finrom_sub(const double* a, const double* b, int64_t count, double* out, void* stream);

/* ---- training the learned error model (deep_learning/dl_model.py:230-243, model.fit) ------------------------------------------ *
 * The network of finrom_mlp_desc trained in fp32 as Keras trains it in the reference: batch normalisation in training form
 * (batch mean, biased batch variance, eps 1e-3; moving <- 0.99 moving + 0.01 batch), loss = mean squared error + l1_l2(1e-4, 1e-4)
 * on W0 and the units' W, Adam in Keras 1.x form (lr_t = lr sqrt(1 - 0.999^t) / (1 - 0.9^t), p -= lr_t m / (sqrt(v) + 1e-7)).
 * The handle owns parameters, Adam's m and v, the moving statistics, the tape and every workspace, all allocated at create
 * (n_w, n_out <= 64, n_layers <= 8 -- FINROM_ERR_UNSUPPORTED beyond; max_batch >= 2): no later call allocates.
 * Host arrays of the set / get calls are fp32 in ONE flat layout, the arrays of ResBnFcModel in this order:
 *     W0 [n_in x n_w], b0 [n_w], then per layer l = 0 .. n_layers (the last one the head):
 *     gamma [n_w], beta [n_w], mean [n_w], var [n_w], W [n_w x n_w] (head: [n_w x n_out]), b [n_w] (head: [n_out])
 * finrom_mlp_train_param_count returns its length.  For m and v the mean / var slots are ignored (read back as zero); for the
 * gradients they carry the step's batch mean and biased batch variance.
 *   _set_params / _get_params   parameters with the moving statistics, m, v (NULL: zero / skipped) and Adam's step count t
 *   _set_lr        the learning rate lives in device memory (the same captured launches serve every epoch); set between replays
 *   _grad          one batch: X [S x n_in], Y [S x n_out] fp32 device arrays that stay resident, rows [B] device int32 row indices
 *                  (the batch is taken by index; the caller checks them against S where it builds the permutation).  Training-form
 *                  forward and backward: every gradient, the batch statistics, loss (with the regulariser) and MAPE
 *                  (100 mean |y - out| / max(|y|, 1e-7)) into the handle.  2 <= B <= max_batch, FINROM_ERR_ARG otherwise.
 *   _apply         Adam on every parameter with the gradients in the handle, the moving statistics, t += 1, and the running sums
 *                  of loss x rows, MAPE x rows, rows, MSE x rows (the loss without the regulariser) that _epoch_stats reads into
 *                  out [4] (and clears when reset != 0)
 *   _get_grads / _set_grads   what _grad left / what _apply will use: gradients (flat layout), loss_mape [2] (doubles);
 *                  _set_grads also takes the row count B that weighs the running sums (its loss stands in for the step's MSE)
 *   _eval          inference form (moving statistics) over X, Y [S x ...] (any S, in pieces of max_batch): out [2] = loss with the
 *                  regulariser, MAPE; synchronises the stream
 * _grad and _apply are launches only -- a linear chain on `stream`, no allocation, no host synchronisation, no atomics, every
 * sum in a fixed order: stream order and graph replay give the same bits, run to run.  An epoch may be captured in one graph
 * (each step's `rows` pointer and B are baked in; the permutation is uploaded into the same buffer before each replay).  The
 * set / get calls, _eval and _epoch_stats synchronise and are refused under capture.  Arguments are checked before any device
 * call.  The trained weights reach finrom_mlp_predict / finrom_romml_grad through _get_params and finrom_mlp_create (scale =
 * gamma / sqrt(var + 1e-3), shift = beta - mean scale, folded by the caller as for any other weights). */
typedef struct finrom_mlp_train_s* finrom_mlp_train_t;
typedef struct {
  int32_t n_in, n_w, n_layers, n_out, max_batch;
} finrom_mlp_train_desc;
int finrom_mlp_train_create(const finrom_mlp_train_desc* desc, finrom_mlp_train_t* out);
void finrom_mlp_train_destroy(finrom_mlp_train_t h);
int64_t finrom_mlp_train_param_count(finrom_mlp_train_t h);
int finrom_mlp_train_set_params(finrom_mlp_train_t h, const float* params, const float* m, const float* v, int64_t t);
int finrom_mlp_train_get_params(finrom_mlp_train_t h, float* params, float* m, float* v, int64_t* t);
int finrom_mlp_train_set_lr(finrom_mlp_train_t h, double lr, void* stream);
int finrom_mlp_train_grad(finrom_mlp_train_t h, const float* X, const float* Y, const int32_t* rows, int32_t B, void* stream);
int finrom_mlp_train_apply(finrom_mlp_train_t h, void* stream);
int finrom_mlp_train_get_grads(finrom_mlp_train_t h, float* grads, double* loss_mape);
int finrom_mlp_train_set_grads(finrom_mlp_train_t h, const float* grads, const double* loss_mape, int32_t B);
int finrom_mlp_train_eval(finrom_mlp_train_t h, const float* X, const float* Y, int64_t S, double* out, void* stream);
int finrom_mlp_train_epoch_stats(finrom_mlp_train_t h, double* out, int32_t reset, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* FINROM_H */
