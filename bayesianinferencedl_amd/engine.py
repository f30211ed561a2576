"""Python-side owners of the library handles.  Each ``solve`` is one C-ABI call that runs the
whole batch on the GPU; inputs may be NumPy arrays (copied to / from the device around the
call) or torch CUDA tensors (used in place, results returned as torch tensors on the same
device, launched on torch's current stream)."""
from __future__ import annotations

import ctypes as C

import numpy as np
import scipy.sparse as sp

from . import _ffi
from ._ffi import FomBandDesc, FomBandGradDesc, FomSmallDesc, DeviceBuffer, FomDesc, FomGradDesc, MlpDesc, RomDesc, check, f64, i32, lib


import os as _os
# LDS row cache of the FOM interpreter: (slots+2) x 512 B per wave.  42 -> 22 KiB, 7 waves per CU (154 KiB);
# 72 -> 37 KiB, 4 waves per CU.  FWD_CHUNK = ops per prefetch chunk of the forward stream (8 or 16).
ROW_CACHE_SLOTS = int(_os.environ.get("FINROM_ROW_CACHE", "40"))
FWD_CHUNK = int(_os.environ.get("FINROM_FWD_CHUNK", "8"))
# Parameter vectors of at most FUSED_X_MAX entries (the five / nine fin conductivities) sit in the interpreter's LDS and
# the op stream assembles A itself (no pre-pass); their slots come out of the row cache so that 7 waves still share a CU.
FUSED_X_MAX = int(_os.environ.get("FINROM_FUSED_X_MAX", "16"))
# Batches of at most SMALL_MAX samples use the latency-oriented schedule: one workgroup per sample, 16 lanes per row of L
# (finrom_fom_set_small) -- for GRADIENTS on every mesh, for forward solves only where no band plan is installed (m >= 32):
# since round 3 the band sweep serves small forward batches too (a lone wave of it: 1.7-2.3 ms at m = 12, 4.2-4.4 ms at m = 20,
# against 2.7 and 17.9 ms here).  0 disables it.  Measured cross-over against the interpreter: ~700 samples at m = 12 (value
# vector in LDS, one workgroup per CU), several thousand at m = 20 (value vector in L2).
SMALL_MAX = int(_os.environ.get("FINROM_SMALL_MAX", "512"))
SMALL_MAX_GLOBAL = int(_os.environ.get("FINROM_SMALL_MAX_GLOBAL", "4096"))
# Batches beyond the small-batch schedule use the frontal band sweep (front in registers, csrc/fom_band.hip) when the mesh
# has a band plan and the library has its window sizes; FINROM_NO_BAND=1 keeps the schedule interpreter.
USE_BAND = _os.environ.get("FINROM_NO_BAND") is None


def _is_torch(x):
    return hasattr(x, "data_ptr") and hasattr(x, "is_cuda")


class DeviceArray:
    """A [S, d] fp64 array that already lives on the device in a library-owned buffer: the output of one call handed to the
    next without a round trip through the host (sub-fin averages -> reduced solve for NumPy callers)."""

    def __init__(self, buf, shape):
        self.buf, self.shape = buf, tuple(shape)


class _Batch:
    """Uniform view of a [S, d] fp64 batch living on the device."""

    def __init__(self, x, d):
        self.torch = _is_torch(x)
        if isinstance(x, DeviceArray):
            assert x.shape[-1] == d, (x.shape, d)
            self.S = int(np.prod(x.shape[:-1]))
            self.keep = x.buf
            self.ptr = x.buf.ptr
            self.stream = None
        elif self.torch:
            import torch
            if not x.is_cuda or x.dtype != torch.float64:
                raise TypeError("torch inputs must be float64 CUDA tensors")
            x = x.reshape(-1, d).contiguous()
            self.keep = x
            self.S = x.shape[0]
            self.ptr = x.data_ptr()
            self.device = x.device
            self.stream = torch.cuda.current_stream(x.device).cuda_stream
        else:
            a = np.ascontiguousarray(x, dtype=np.float64).reshape(-1, d)
            self.S = a.shape[0]
            self.keep = DeviceBuffer.from_numpy(a)
            self.ptr = self.keep.ptr
            self.stream = None

    # NumPy callers: the outputs of one library call are carved from shared arenas (one zero-fill, ONE copy back for all of
    # them) -- a one-sample call is dominated by driver round trips, not by the kernels (the MAP / HMC pattern of configs[4]).
    _ARENA_MIN = 64 << 10

    def new(self, shape, dtype="f8", zero=True):
        """Allocate an output of the same kind, zero-filled unless the call overwrites all of it (zero=False: one fill kernel
        less per output on the torch path -- they add up in a one-sample call); returns (handle, device pointer).
        info is always zero-filled: every entry point ORs its flags into it (include/finrom.h, Conventions) but finrom_romml_grad,
        which overwrites it and is the one call that gets zero=False for it."""
        if self.torch:
            import torch
            t = (torch.zeros if zero else torch.empty)(shape, dtype=torch.float64 if dtype == "f8" else torch.int32, device=self.device)
            return t, t.data_ptr()
        n = int(np.prod(shape)) * (8 if dtype == "f8" else 4)
        arenas = self.__dict__.setdefault("_arenas", [])
        need = (n + 255) // 256 * 256
        if not arenas or arenas[-1][1] + need > arenas[-1][0].nbytes:
            buf = DeviceBuffer(max(need, self._ARENA_MIN if n <= self._ARENA_MIN else need))
            buf.zero()
            arenas.append([buf, 0, None])                  # [device buffer, bytes used, host copy]
        a = arenas[-1]
        off = a[1]
        a[1] += need
        return (len(arenas) - 1, off, n), a[0].ptr + off

    def out(self, obj, shape, dtype="f8"):
        if self.torch:
            return obj
        ia, off, n = obj
        a = self._arenas[ia]
        if a[2] is None:                                    # first read after the call: one copy of what the arena holds
            a[2] = a[0].to_numpy((max(a[1], 8),), np.uint8)
        return a[2][off:off + n].view(np.float64 if dtype == "f8" else np.int32).reshape(shape)


def _sync_if_mixed(b, other):
    """A torch-stream call that also consumed a NumPy operand staged through a pooled DeviceBuffer: the kernels may still be
    running on torch's (non-blocking) stream when that buffer goes back to the library's pool and its next owner writes it on the
    default stream.  The staging buffer remembers the launch stream: it is parked behind an event recorded there
    (finrom_free_async) and the next owner waits for that event -- no host synchronisation here."""
    if b.torch and not other.torch and isinstance(other.keep, DeviceBuffer):
        other.keep.used_on(b.stream)


def _csr_rows(M):
    M = sp.csr_matrix(M)
    M.sort_indices()
    return M.indptr.astype(np.int32), M.indices.astype(np.int32), M.data.astype(np.float64)


class FomEngine:
    """Batched ``A(x) w = F`` + QoI (finrom_fom_*).  ``c0``/``W`` define the sparse-affine
    value map on the CSR pattern of A (see include/finrom.h)."""

    def __init__(self, plan, c0_csr, W_csr, rhs, B_obs, pattern=None, ops=None):
        self.plan = plan
        self.band = None
        self.band_mirror = None             # half-domain plan of a mirror-symmetric operator (calls without w), if installed
        self.n = plan.n
        W_csr = sp.csr_matrix(W_csr)
        self.xdim = W_csr.shape[1]
        self._W, self._pattern, self._grad = W_csr, pattern, False
        c0, aptr, aidx, aw = plan.entry_table(c0_csr, W_csr)
        Bp = sp.csr_matrix(np.asarray(B_obs)[:, plan.perm]) if not sp.issparse(B_obs) else sp.csr_matrix(B_obs)[:, plan.perm]
        self._Bp = Bp
        optr, oidx, ow = _csr_rows(Bp)
        self.n_obs = Bp.shape[0]
        keep = []

        def I(a):
            a, p = i32(a); keep.append(a); return p

        def D(a):
            a, p = f64(a); keep.append(a); return p

        fused = self.xdim <= min(FUSED_X_MAX, 16) and ROW_CACHE_SLOTS - self.xdim >= 8
        slots = ROW_CACHE_SLOTS - (self.xdim if fused else 0)
        streams = plan.op_streams(slots, np.asarray(rhs)[plan.perm], FWD_CHUNK, (c0, aptr, aidx, aw) if fused else None)
        self.cache_slots, self.fused, self._streams = slots, fused, streams
        fk, fa, fb, fd = streams["fwd"]; bk, ba, bb, bd = streams["bwd"]
        d = FomDesc(n=plan.n, nnzL=plan.nnzL, xdim=self.xdim, n_obs=self.n_obs, nasm=len(aidx),
                    n_alist=len(streams["a_list"]), cache_slots=slots, fwd_chunk=FWD_CHUNK, nops_fwd=len(fk), nops_bwd=len(bk),
                    a_list=I(streams["a_list"]), asm_c0=D(c0), asm_ptr=I(aptr), asm_idx=I(aidx), asm_w=D(aw),
                    rhs=D(np.asarray(rhs)[plan.perm]),
                    fwd_kind=I(fk), fwd_a=I(fa), fwd_b=I(fb), fwd_d=I(fd),
                    bwd_kind=I(bk), bwd_a=I(ba), bwd_b=I(bb), bwd_d=I(bd),
                    obs_ptr=I(optr), obs_idx=I(oidx), obs_w=D(ow), perm=I(plan.perm),
                    n_imm=len(streams["imm"]), imm=D(streams["imm"]))
        h = C.c_void_p()
        check(lib().finrom_fom_create(C.byref(d), C.byref(h)), "finrom_fom_create")
        self._h = h
        if SMALL_MAX > 0:
            lpf, lrf, lpb, lrb = plan.level_sets()
            in_lds = (plan.nnzL + 3 * plan.n + self.xdim) * 8 <= 156 * 1024          # the library's own criterion
            sd = FomSmallDesc(small_max=SMALL_MAX if in_lds else SMALL_MAX_GLOBAL, npairs=plan.npairs, nasm=len(aidx), nlev_f=len(lpf) - 1, nlev_b=len(lpb) - 1,
                              row_ptr=I(plan.row_ptr), ent_col=I(plan.ent_col),
                              pair_ptr=I(plan.pair_ptr), pair_a=I(plan.pair_a), pair_b=I(plan.pair_b),
                              asm_c0=D(c0), asm_ptr=I(aptr), asm_idx=I(aidx), asm_w=D(aw),
                              col_ptr=I(plan.col_ptr), col_ent=I(plan.col_ent), col_row=I(plan.col_row),
                              lev_ptr_f=I(lpf), lev_rows_f=I(lrf), lev_ptr_b=I(lpb), lev_rows_b=I(lrb))
            check(lib().finrom_fom_set_small(self._h, C.byref(sd)), "finrom_fom_set_small")
        if USE_BAND and ops is not None:
            self._enable_band(ops, c0_csr, W_csr, rhs, B_obs)

    @staticmethod
    def band_descriptor(bp, xdim, c0_csr, W_csr, rhs, B_obs):
        """finrom_fom_band_desc of band plan `bp` for one operator table -> (descriptor, arrays it borrows, physical slots)."""
        c0, ptr, idx, w = bp.ab_table(c0_csr, W_csr)
        abmap, c0p, ptrp, idxp, wp = bp.compact_slots(c0, ptr, idx, w)      # logical -> physical value slots (duplicates shared)
        F = np.asarray(rhs, dtype=np.float64)
        if bp.rhs_scale is not None:                     # half plan: the centre line's load is halved (bandplan.py)
            F = F.copy(); F[bp.perm] *= bp.rhs_scale
        Fg = np.zeros(bp.G)
        for seg in bp.fin_segs + [bp.post_seg]:
            Fg[seg.g0:seg.g0 + seg.npiv] = F[bp.perm[seg.e0:seg.e0 + seg.npiv]]
        Bp = sp.csr_matrix(np.asarray(B_obs)[:, bp.perm]) if not sp.issparse(B_obs) else sp.csr_matrix(B_obs)[:, bp.perm]
        optr, oidx, ow = _csr_rows(Bp)
        nif = bp.q + 1
        schur = np.asarray([[abmap[off] for _, _, off in tg] for tg in bp.schur_target], np.int32)
        qo = FomEngine.qoi_only_tables(bp, Bp, Fg)
        keep = []

        def I(a):
            a, p = i32(a); keep.append(a); return p

        def D(a):
            a, p = f64(a); keep.append(a); return p
        d = FomBandDesc(NSF=bp.NSF, NSP=bp.NSP, NX=bp.NX, nfins=bp.nfins, npf=bp.npf, nif=nif, npost=bp.npost, nAB=len(c0p),
                        nterms=len(idxp), nLx=bp.nLx, ab_c0=D(c0p), ab_ptr=I(ptrp), ab_idx=I(idxp), ab_w=D(wp), abmap=I(abmap[:3 * bp.G]),
                        Fg=D(Fg), act=I(bp.act), lx_ptr=I(bp.lx_ptr), ent_extra=I(bp.ent_extra),
                        ecp_ptr=I(bp.ecp_ptr), ecp_slot=I(bp.ecp_slot), ecp_off=I(abmap[bp.ecp_off] if len(bp.ecp_off) else bp.ecp_off),
                        schur_off=I(schur), iface_elim=I(bp.iface_elim),
                        perm=I(np.arange(bp.n) if bp.mirror else bp.perm),      # (the half plan serves no call that unpacks w)
                        obs_ptr=I(optr), obs_idx=I(oidx), obs_w=D(ow))
        if qo is not None:
            FgQ, row_fin, qptr, qidx, qw = qo
            d.qoi_FgQ, d.qoi_row_fin, d.qoi_obs_ptr, d.qoi_obs_idx, d.qoi_obs_w = D(FgQ), I(row_fin), I(qptr), I(qidx), D(qw)
        return d, keep, len(c0p)

    @staticmethod
    def qoi_only_tables(bp, Bp, Fg):
        """Tables of the band sweep's QoI-only form (include/finrom.h, finrom_fom_band_desc::qoi_*): every observation row is
        split into the weights on ONE fin's segment nodes (own + interface: they ride through that fin's forward sweep as its
        right-hand side) and a post-only remainder.  None when the observation operator does not split that way (a row with
        weights on the own nodes of two fins, two rows on one fin -- e.g. the 40 point observations of external_obs -- or a load
        on the fins): the full sweep then serves every call."""
        Bp = sp.csr_matrix(Bp)
        n_obs = Bp.shape[0]
        npf, nfins, nif = bp.npf, bp.nfins, bp.q + 1
        ntot, post_e0 = npf + nif, nfins * npf
        if np.any(Fg[:nfins * ntot] != 0.0):
            return None
        row_fin = np.full(n_obs, -1, np.int32)
        fin_row = np.full(nfins, -1, np.int64)
        for o in range(n_obs):
            idx = Bp.indices[Bp.indptr[o]:Bp.indptr[o + 1]]
            fins = np.unique(idx[idx < post_e0] // npf)
            if len(fins) > 1:
                return None
            if len(fins) == 1:
                if fin_row[fins[0]] >= 0:
                    return None
                row_fin[o], fin_row[fins[0]] = fins[0], o
        FgQ = np.array(Fg, dtype=np.float64, copy=True)
        qptr, qidx, qw = [0], [], []
        for o in range(n_obs):
            idx = Bp.indices[Bp.indptr[o]:Bp.indptr[o + 1]]; val = Bp.data[Bp.indptr[o]:Bp.indptr[o + 1]]
            f = int(row_fin[o])
            iface = {int(e): t for t, e in enumerate(bp.iface_elim[f])} if f >= 0 else {}
            for e, v in zip(idx, val):
                e = int(e)
                if e < post_e0:
                    FgQ[f * ntot + (e - f * npf)] = v
                elif e in iface:
                    FgQ[f * ntot + npf + iface[e]] = v
                else:
                    qidx.append(e); qw.append(v)
            qptr.append(len(qidx))
        return FgQ, row_fin, np.asarray(qptr, np.int32), np.asarray(qidx, np.int32), np.asarray(qw, np.float64)

    def _enable_band(self, ops, c0_csr, W_csr, rhs, B_obs):
        """Install the frontal band sweep (finrom_fom_set_band) when the mesh has a band plan and the library was built with
        its window sizes; otherwise the handle keeps the interpreter."""
        bp = ops.band_plan()
        if bp is None:
            return
        d, keep, nslots = self.band_descriptor(bp, self.xdim, c0_csr, W_csr, rhs, B_obs)
        rc = lib().finrom_fom_set_band(self._h, C.byref(d))
        if rc == -4:                                     # FINROM_ERR_UNSUPPORTED: window sizes not built in -> interpreter
            return
        check(rc, "finrom_fom_set_band")
        self.band = bp
        self._B_band = sp.csr_matrix(np.asarray(B_obs)[:, bp.perm]) if not sp.issparse(B_obs) else sp.csr_matrix(B_obs)[:, bp.perm]
        self.band_slots = nslots            # physical value slots per sample (bench: algorithmic bytes)
        self.band_qoi_only = bool(d.qoi_FgQ)      # calls without w: QoI-only form
        self._enable_mirror(ops, c0_csr, W_csr, rhs, B_obs)

    @staticmethod
    def mirror_rows(ops, c0_csr, W_csr, rhs, B_obs, tol=1e-13, col_twin=None):
        """Is this operator table mirror-symmetric about x = 3?  With P the mesh's mirror permutation (bandplan.mirror_permutation)
        and the pattern entry (a, b) mapped to (P a, P b): `c0`, every column of `W` (the PARAMETERS stay where they are: a nodal
        field or nine fin conductivities are not symmetric, the five-parameter lift is), `rhs`, and the rows of `B_obs`, each
        of which must map onto a row.  Tolerance `tol` relative to each table's largest magnitude; the tables of the lattice
        mesh are symmetric to 4.4e-15 in that measure (m = 12: c0 4.1e-15, W 2.0e-15, B_obs 4.4e-15, F exactly; m = 4, 8: <= 2e-16).
        `col_twin` (the reduced model's test, RomEngine.set_mirror): column p of `W` must map onto column col_twin[p] instead --
        parameters that mirror each other, for samples that carry the same value in both.
        -> twin[o] = the row that mirrors row o (twin[o] == o: a self-mirrored row), or None."""
        from .bandplan import mirror_permutation
        n = ops.n
        P = mirror_permutation(ops.mesh)
        indptr, indices = np.asarray(ops.indptr), np.asarray(ops.indices)
        rows = np.repeat(np.arange(n), np.diff(indptr))
        key = rows.astype(np.int64) * n + indices
        order = np.argsort(key, kind="stable")
        mkey = P[rows] * n + P[indices]
        pos = np.searchsorted(key[order], mkey)
        if np.any(pos >= len(key)) or np.any(key[order][np.minimum(pos, len(key) - 1)] != mkey):
            return None                                   # the pattern itself is not mirror-symmetric
        pe = order[pos]                                   # entry (a, b) -> entry (P a, P b)

        def same(a, b):
            a, b = (sp.csr_matrix(a), sp.csr_matrix(b)) if sp.issparse(a) or sp.issparse(b) else (np.asarray(a, float), np.asarray(b, float))
            scale = abs(a).max()
            return scale == 0.0 or abs(a - b).max() <= tol * scale
        c0 = np.asarray(c0_csr, dtype=np.float64)
        W = sp.csr_matrix(W_csr)
        F = np.asarray(rhs, dtype=np.float64)
        Wm = W[pe] if col_twin is None else W[pe][:, np.asarray(col_twin)]
        if not (same(c0, c0[pe]) and same(W, Wm) and same(F, F[P])):
            return None
        B = B_obs.toarray() if sp.issparse(B_obs) else np.asarray(B_obs, dtype=np.float64)
        Bm, scale = B[:, P], np.abs(B).max()
        twin = np.full(B.shape[0], -1, np.int64)
        for o in range(B.shape[0]):
            hit = np.nonzero(np.abs(B - Bm[o][None, :]).max(axis=1) <= tol * scale)[0]
            if len(hit) != 1:
                return None
            twin[o] = hit[0]
        if np.any(twin[twin] != np.arange(len(twin))):
            return None
        return twin

    @staticmethod
    def mirror_tables(ops, bp, B_obs, twin):
        """Observation operator of the half problem.  For a mirror-symmetric w, row o is  sum_l (B[o, l] + B[o, P l]) w_l  over
        the left nodes plus its own weights on the centre line: a row that lives on a left fin stays as it is, a self-mirrored
        row (the post's) is folded, and the right-hand twin of a row is not computed at all -- it is a copy.
        -> (B_half [rows x n_mesh] in dof columns, out_ptr, out_col: the output columns of each computed row)."""
        B = B_obs.toarray() if sp.issparse(B_obs) else np.asarray(B_obs, dtype=np.float64)
        P = bp.mirror_of
        left = bp.perm[bp.rhs_scale == 1.0]
        reps = [o for o in range(len(twin)) if o <= twin[o]]
        Bh = np.zeros((len(reps), B.shape[1]))
        Bh[:, bp.perm] = B[reps][:, bp.perm]
        Bh[:, left] += B[reps][:, P[left]]
        out_ptr, out_col = [0], []
        for o in reps:
            out_col += [o] if twin[o] == o else [o, int(twin[o])]
            out_ptr.append(len(out_col))
        return Bh, np.asarray(out_ptr, np.int32), np.asarray(out_col, np.int32)

    @staticmethod
    def mirror_form(ops, xdim, c0_csr, W_csr, rhs, B_obs):
        """The half-domain form of one operator table, or None: the table must be mirror-symmetric (mirror_rows), the mesh must
        have a half plan and the half operator QoI-only tables (the half plan serves calls without w only).
        -> (half plan, its finrom_fom_band_desc, arrays the descriptor borrows, physical slots, out_ptr, out_col)."""
        bpm = ops.band_plan_mirror() if hasattr(ops, "band_plan_mirror") else None
        if bpm is None:
            return None
        twin = FomEngine.mirror_rows(ops, c0_csr, W_csr, rhs, B_obs)
        if twin is None:
            return None
        Bh, out_ptr, out_col = FomEngine.mirror_tables(ops, bpm, B_obs, twin)
        d, keep, nslots = FomEngine.band_descriptor(bpm, xdim, c0_csr, W_csr, rhs, Bh)
        if not d.qoi_FgQ:
            return None
        return bpm, d, keep, nslots, out_ptr, out_col

    def _enable_mirror(self, ops, c0_csr, W_csr, rhs, B_obs):
        """Install the half-domain plan for calls that want no w (finrom_fom_set_band_mirror) when the operator table is
        mirror-symmetric (mirror_rows), the half operator has QoI-only tables and the library has the half plan's window sizes.
        Otherwise nothing changes.  FINROM_NO_MIRROR=1 at engine creation switches the form off."""
        self.band_mirror = None
        self.band_mirror_form = 0
        self.band_mirror_records = False
        if _os.environ.get("FINROM_NO_MIRROR") is not None or not self.band_qoi_only:
            return
        form = self.mirror_form(ops, self.xdim, c0_csr, W_csr, rhs, B_obs)
        if form is None:
            return
        bpm, d, keep, nslots, out_ptr, out_col = form
        op, oc = i32(out_ptr), i32(out_col)
        rc = lib().finrom_fom_set_band_mirror(self._h, C.byref(d), bpm.n, len(out_ptr) - 1, op[1], oc[1])
        if rc == -4:                                     # window sizes not built in
            return
        check(rc, "finrom_fom_set_band_mirror")
        self.band_mirror = bpm
        self.band_mirror_slots = nslots
        # 2: the post's observation rows ride its forward sweep as functionals (no stored factor); 1: the stored-factor form --
        # a descriptor that does not fit the functional form, or FINROM_FOM_POST_STORED=1 at engine creation
        self.band_mirror_form = int(lib().finrom_fom_band_mirror_form(self._h))
        # the functional form's sweeps read one prefetched record per pivot (FINROM_FOM_NO_PIVOT_RECORDS=1 at engine creation: the
        # tables themselves, same bits)
        self.band_mirror_records = bool(lib().finrom_fom_band_mirror_records_on(self._h))

    def solve(self, X, want_w=False):
        b = _Batch(X, self.xdim)
        S = b.S
        qoi, qp = b.new((S, self.n_obs))
        info, ip = b.new((S,), "i4")
        w, wp = (b.new((S, self.n)) if want_w else (None, None))
        check(lib().finrom_fom_solve(self._h, b.ptr, S, qp, wp, ip, b.stream), "finrom_fom_solve")
        return {"qoi": b.out(qoi, (S, self.n_obs)), "w": b.out(w, (S, self.n)) if want_w else None,
                "info": b.out(info, (S,), "i4")}

    def last_path(self):
        """Name of the schedule the most recent solve / gradient on this handle launched (finrom_fom_last_path):
        'small_lds', 'small_global', 'interpreter', 'band_registers', 'band_lds_4wave' ('none' before the first call)."""
        rc = lib().finrom_fom_last_path(self._h)
        if rc < 0:
            check(rc, "finrom_fom_last_path")
        return _ffi.FOM_PATHS[rc]

    def set_small_max(self, small_max):
        """Move the batch-size threshold of the small-batch schedule (0: every batch takes the throughput path)."""
        check(lib().finrom_fom_set_small_max(self._h, int(small_max)), "finrom_fom_set_small_max")

    def solve_rhs(self, X, rhs):
        """X [S, xdim], rhs [S, nrhs, n] (dof order) -> dict(out [S, nrhs, n] = A(x_s)^-1 rhs, info [S]) (finrom_fom_solve_rhs)."""
        b = _Batch(X, self.xdim)
        S = b.S
        rhs = rhs if _is_torch(rhs) else np.ascontiguousarray(rhs, dtype=np.float64)
        nrhs = int(rhs.shape[-2]) if rhs.ndim == 3 else 1
        rb = _Batch(rhs, nrhs * self.n)
        assert rb.S == S, (rb.S, S)
        out, op = b.new((S, nrhs, self.n), zero=False) if b.torch else b.new((S, nrhs, self.n))
        info, ip = b.new((S,), "i4")
        check(lib().finrom_fom_solve_rhs(self._h, b.ptr, S, rb.ptr, nrhs, op, ip, b.stream), "finrom_fom_solve_rhs")
        _sync_if_mixed(b, rb)
        return {"out": b.out(out, (S, nrhs, self.n)), "info": b.out(info, (S,), "i4")}

    def _enable_gradient(self):
        """One-time tables of the adjoint gradient (finrom_fom_set_gradient)."""
        if self._grad:
            return
        if self._pattern is None:
            raise ValueError("FomEngine needs the CSR pattern of A for gradients")
        from .symbolic import build_resolve_stream
        plan, n = self.plan, self.n
        rk, ra, rb, rd = build_resolve_stream(plan, plan.nnzL + 2 * n)
        Bt = sp.csr_matrix(self._Bp.T)                       # [n(permuted) x n_obs]
        Bt.sort_indices()
        indptr, indices = np.asarray(self._pattern[0]), np.asarray(self._pattern[1])
        e_row = np.repeat(np.arange(n), np.diff(indptr))
        Wt = sp.csc_matrix(self._W)                          # columns = parameters
        g_ptr = Wt.indptr.astype(np.int32)
        ent = Wt.indices
        g_a = plan.iperm[e_row[ent]].astype(np.int32)        # row of the entry, permuted
        g_b = plan.iperm[indices[ent]].astype(np.int32)      # column of the entry, permuted
        keep = []

        def I(a):
            a, p = i32(a); keep.append(a); return p

        def D(a):
            a, p = f64(a); keep.append(a); return p

        d = FomGradDesc(nops_res=len(rk), res_kind=I(rk), res_a=I(ra), res_b=I(rb), res_d=I(rd),
                        bt_ptr=I(Bt.indptr), bt_obs=I(Bt.indices), bt_w=D(Bt.data),
                        g_ptr=I(g_ptr), g_a=I(g_a), g_b=I(g_b), g_w=D(Wt.data))
        check(lib().finrom_fom_set_gradient(self._h, C.byref(d)), "finrom_fom_set_gradient")
        if self.band is not None:
            # the same tables over the band plan's elimination indices: large batches solve the adjoint on the band layout
            bp = self.band
            Btb = sp.csr_matrix(self._B_band.T)
            Btb.sort_indices()
            gb = FomBandGradDesc(bt_ptr=I(Btb.indptr), bt_obs=I(Btb.indices), bt_w=D(Btb.data), g_ptr=I(g_ptr),
                                 g_a=I(bp.iperm[e_row[ent]]), g_b=I(bp.iperm[indices[ent]]), g_w=D(Wt.data))
            check(lib().finrom_fom_set_band_gradient(self._h, C.byref(gb)), "finrom_fom_set_band_gradient")
        self._grad = True

    def gradient(self, X, data):
        """X [S, xdim], data [n_obs] or [S, n_obs] -> dict(grad [S, xdim], J [S], qoi, info)
        (Fin.gradient, fom/forward_solve.py:293-322, for a batch)."""
        self._enable_gradient()
        b = _Batch(X, self.xdim)
        S = b.S
        data = data if _is_torch(data) else np.ascontiguousarray(data, dtype=np.float64)
        per_sample = 1 if data.ndim == 2 else 0
        db = _Batch(data, self.n_obs)
        grad, gp = b.new((S, self.xdim)); J, Jp = b.new((S,)); qoi, qp = b.new((S, self.n_obs)); info, ip = b.new((S,), "i4")
        check(lib().finrom_fom_gradient(self._h, b.ptr, db.ptr, per_sample, S, gp, Jp, qp, ip, b.stream), "finrom_fom_gradient")
        _sync_if_mixed(b, db)
        return {"grad": b.out(grad, (S, self.xdim)), "J": b.out(J, (S,)), "qoi": b.out(qoi, (S, self.n_obs)),
                "info": b.out(info, (S,), "i4")}

    def close(self):
        if getattr(self, "_h", None):
            _ffi.destroy_handle("finrom_fom_destroy", self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class RomEngine:
    """Batched LSPG reduced solve (finrom_rom_*).

    ``terms``: list of (theta_index, sparse-or-dense [n, r] matrix Psi_p = A_p Phi); theta_index 0 is the
    constant (Robin) term, 1..P the parameters.  Only the non-zero rows of each Psi_p are shipped."""

    @staticmethod
    def pack_terms(n, r, terms):
        """(row_ptr [n + 1], term_p [nterms], term_val [nterms, r]) of finrom_rom_desc: per row of psi its non-zero terms."""
        rows = [[] for _ in range(n)]
        for p, M in terms:
            M = np.asarray(M)
            nzr = np.nonzero(np.abs(M).sum(1))[0]
            for j in nzr:
                rows[j].append((p, M[j]))
        row_ptr = np.zeros(n + 1, np.int32)
        term_p, term_val = [], []
        for j in range(n):
            for p, v in rows[j]:
                term_p.append(p); term_val.append(v)
            row_ptr[j + 1] = len(term_p)
        return row_ptr, term_p, np.asarray(term_val, dtype=np.float64).reshape(len(term_p), r)

    def __init__(self, n, r, P, terms, rhs, obs_phi):
        self.n, self.r, self.P = n, r, P
        row_ptr, term_p, tv = self.pack_terms(n, r, terms)
        self.nterms = len(term_p)
        obs_phi = np.ascontiguousarray(obs_phi, dtype=np.float64)
        self.n_obs = obs_phi.shape[0]
        a1, p1 = i32(row_ptr); a2, p2 = i32(term_p); a3, p3 = f64(tv); a4, p4 = f64(rhs); a5, p5 = f64(obs_phi)
        d = RomDesc(n=n, r=r, P=P, n_obs=self.n_obs, nterms=self.nterms, row_ptr=p1, term_p=p2, term_val=p3,
                    rhs=p4, obs_phi=p5)
        h = C.c_void_p()
        check(lib().finrom_rom_create(C.byref(d), C.byref(h)), "finrom_rom_create")
        self._h = h
        self.mirror_eps = None                            # set_mirror: the gate's measured value (dropped rows counted)
        self.mirror_eps_all_rows = None                   # ... and the value without dropped rows
        self.mirror_dropped = 0                           # rows the installed half list leaves out (mirror_skip_rows)
        self.mirror_dropped_max = 0.0                     # ... and the largest of them, relative to the largest row
        self.mirror_eps_compact = None                    # ... and the gate's value of the compact list, if installed
        self.mirror = False

    # ---- the half form of a mirror-symmetric reduced model (DESIGN 4b', finrom_rom_set_mirror) ----------------------------------
    MIRROR_EPS_GATE = 1e-9       # relative, energy norm: what a list may cost as a FORM.  (The tests hold each list to the
    #                              extended-precision LSPG of its own rows, tests/rom_lspg_cases.py; the lists' own solutions differ
    #                              from the full model's by 1.5e-14 in qoi_r at the sizes tested, tests/test_rom_lspg_host.py.)
    MIRROR_PROBES = 16
    MIRROR_PROBE_RANGE = (0.1, 10.0)       # the dataset's range: where the probes lie, and where the short list is offered

    @staticmethod
    def mirror_probe_eps(tables, perm, theta_twin, nprobe=16, seed=0, low=MIRROR_PROBE_RANGE[0], high=MIRROR_PROBE_RANGE[1], drop=None,
                         rotated=None):
        """How far from mirror-symmetric is the basis, in the metric that matters?  tables[p] = A_p Phi (p = 0: the constant
        term); with perm the mesh's mirror permutation and theta_twin the parameters' (0-based), A_p Phi_s = (tables[p] +
        tables[twin p][perm]) / 2 and A_p Phi_a is the rest.  For mirror-symmetric theta psi^T psi = A_s + D with A_s = psi_s^T psi_s
        and D = psi_a^T psi_a (the cross terms vanish); dropping D changes w_r by at most eps = lambda_max(D, A_s) relative in the
        energy norm.  -> the largest eps over `nprobe` seeded probes, log-uniform over [low, high] per mirror pair.
        drop (bool per row of the FULL mesh, closed under perm): rows of psi_s the half list leaves out as well (mirror_skip_rows);
        their sum joins D and leaves A_s: eps = lambda_max(psi_a^T psi_a + psi_s[drop]^T psi_s[drop], psi_s[kept]^T psi_s[kept]).
        rotated (the compact list, mirror_compact_rows): (kept, truncated), each the tables [P + 1][rows, r] of weighted rows that
        stand for psi_s[kept]; the kept ones form A_s, the truncated ones join D as well."""
        import scipy.linalg as sla
        P = len(theta_twin)
        tw1 = np.concatenate([[0], np.asarray(theta_twin) + 1])
        Ts = [0.5 * (np.asarray(tables[p]) + np.asarray(tables[tw1[p]])[perm]) for p in range(P + 1)]
        Ta = [np.asarray(tables[p]) - Ts[p] for p in range(P + 1)]
        rng = np.random.default_rng(seed)
        worst = 0.0
        for _ in range(nprobe):
            th = np.exp(rng.uniform(np.log(low), np.log(high), P))
            th = th[np.minimum(np.arange(P), np.asarray(theta_twin))]          # the same value in both of a pair
            th1 = np.concatenate([[1.0], th])
            ps = sum(th1[p] * Ts[p] for p in range(P + 1)); pa = sum(th1[p] * Ta[p] for p in range(P + 1))
            D = pa.T @ pa
            if drop is not None:
                D = D + ps[drop].T @ ps[drop]
                ps = ps[~drop]
            if rotated is not None:
                ps = sum(th1[p] * rotated[0][p] for p in range(P + 1)); pt = sum(th1[p] * rotated[1][p] for p in range(P + 1))
                D = D + pt.T @ pt
            try:
                L = np.linalg.cholesky(ps.T @ ps)
            except np.linalg.LinAlgError:                   # psi_s alone is rank-deficient: nothing like a symmetric basis
                return float("inf"), Ts
            M = sla.solve_triangular(L, sla.solve_triangular(L, D, lower=True).T, lower=True)
            worst = max(worst, float(np.linalg.eigvalsh(0.5 * (M + M.T)).max()))
        return worst, Ts

    @staticmethod
    def mirror_descriptor(n, r, P, Ts, rows, weight, theta_twin, rhs, dropped=None):
        """The half descriptor: rows `rows` (left of the symmetry line: weight 2, on it: weight 1) of the symmetrised tables Ts,
        the two tables of a mirror pair merged under the smaller index (the samples that use it carry the same value in both);
        rhs = weight F.  dropped (bool per half row, mirror_skip_rows): these rows stay in the descriptor with node and weight but
        get no terms (row_ptr[i + 1] == row_ptr[i]), so no k-step multiplies them.
        -> (finrom_rom_desc, the arrays it borrows, row_node, row_weight, theta_twin as ctypes pairs)."""
        rows = np.asarray(rows, np.int64)
        merged = []
        for p in range(P + 1):
            t = 0 if p == 0 else int(theta_twin[p - 1]) + 1
            if t < p:
                continue
            M = Ts[p][rows] if t == p else Ts[p][rows] + Ts[t][rows]
            if dropped is not None and np.any(dropped):
                M = np.where(np.asarray(dropped, bool)[:, None], 0.0, M)
            merged.append((p, M))
        row_ptr, term_p, tv = RomEngine.pack_terms(len(rows), r, merged)
        keep = [i32(row_ptr), i32(term_p), f64(tv), f64(np.asarray(weight, float) * np.asarray(rhs, float)[rows]),
                i32(rows), f64(weight), i32(theta_twin)]
        d = RomDesc(n=len(rows), r=r, P=P, n_obs=0, nterms=len(term_p), row_ptr=keep[0][1], term_p=keep[1][1], term_val=keep[2][1],
                    rhs=keep[3][1], obs_phi=None)
        return d, keep

    MIRROR_SKIP_TAUS = (1e-6, 1e-7, 1e-8, 1e-9)       # row-size thresholds tried in this order (mirror_skip_rows)

    @staticmethod
    def mirror_skip_rows(tables, Ts, rhs, perm, rows, theta_twin):
        """Which rows of the half list are zero up to rounding for EVERY theta (DESIGN 4b'', the discrete-harmonic rows: a node whose
        patch lies inside one sub-domain and off the Robin boundary has (K_d w)_i = 0 for every snapshot w, hence for every POD
        vector)?  Row size rn_i = sqrt(sum_p |Ts[p][i]|^2); candidates are the rows with rn_i <= tau max rn that carry no load.  The
        first tau of MIRROR_SKIP_TAUS whose combined probe value -- mirror_probe_eps with the candidates (and their twins) moved
        from A_s to D -- is at most MIRROR_EPS_GATE decides.  -> (dropped: bool per half row, combined eps, tau, the largest dropped
        rn_i / max rn) or (all False, None, None, 0.0) when no tau passes or none has a candidate."""
        rows = np.asarray(rows, np.int64)
        rn = np.sqrt(sum((np.asarray(T)[rows] ** 2).sum(axis=1) for T in Ts))
        none = np.zeros(len(rows), bool)
        if not rn.max() > 0.0:
            return none, None, None, 0.0
        loaded = np.asarray(rhs, float)[rows] != 0.0
        for tau in RomEngine.MIRROR_SKIP_TAUS:
            cand = (rn <= tau * rn.max()) & ~loaded
            if not cand.any():
                break
            drop = np.zeros(np.asarray(perm).shape[0], bool)
            drop[rows[cand]] = True
            drop[np.asarray(perm)[rows[cand]]] = True
            eps = RomEngine.mirror_probe_eps(tables, perm, theta_twin, nprobe=RomEngine.MIRROR_PROBES, drop=drop)[0]
            if eps <= RomEngine.MIRROR_EPS_GATE:
                return cand, eps, tau, float(rn[cand].max() / rn.max())
        return none, None, None, 0.0

    MIRROR_COMPACT_TAUS = (1e-8, 1e-9, 1e-10)      # singular-value thresholds tried in this order (mirror_compact_rows)

    @staticmethod
    def compact_rows(desc, keep, tau, with_q=False):
        """finrom_rom_compact_rows on a short descriptor (mirror_descriptor's pair) -> dict(tv [nterms, r], rhs [n], cls [n], sigma
        [n], keep [n], sigma_max, Q [n, n] or None): the rows times sqrt(weight), rotated per pattern class where that saves a
        k-step at this tau."""
        n, r = desc.n, desc.r
        out = {"tv": np.zeros((desc.nterms, r)), "rhs": np.zeros(n), "cls": np.zeros(n, np.int32), "sigma": np.zeros(n),
               "keep": np.zeros(n, np.int32), "Q": np.zeros((n, n)) if with_q else None}
        smax = C.c_double()
        ptr = lambda a, t: a.ctypes.data_as(t)
        check(lib().finrom_rom_compact_rows(C.byref(desc), keep[5][1], float(tau), ptr(out["tv"], _ffi.c_f64p), ptr(out["rhs"], _ffi.c_f64p),
                                            ptr(out["cls"], _ffi.c_i32p), ptr(out["sigma"], _ffi.c_f64p), ptr(out["keep"], _ffi.c_i32p),
                                            ptr(out["Q"], _ffi.c_f64p) if with_q else None, n if with_q else 0, C.byref(smax)),
              "finrom_rom_compact_rows")
        out["sigma_max"] = smax.value
        return out

    @staticmethod
    def compact_tables(desc, keep, out, P):
        """(kept, truncated): the compact rows of compact_rows as tables [P + 1][rows, r] (mirror_probe_eps's `rotated`)."""
        row_ptr, term_p = np.asarray(keep[0][0]), np.asarray(keep[1][0])
        T = np.zeros((P + 1, desc.n, desc.r))
        T[term_p, np.repeat(np.arange(desc.n), np.diff(row_ptr))] = out["tv"]
        kept = out["keep"] != 0
        return T[:, kept], T[:, ~kept]

    @staticmethod
    def mirror_compact_rows(tables, perm, theta_twin, rows, dropped_rows, desc, keep):
        """The compact list of a short descriptor (DESIGN 4b'', finrom_rom_compact_rows): per pattern class the rows rotated onto the
        singular directions of the class's stacked tables, the rotated rows below tau x the largest singular value over all classes
        without terms.  The first tau of MIRROR_COMPACT_TAUS whose combined probe value -- mirror_probe_eps with psi_a^T psi_a, the
        short list's dropped rows and the truncated rotated rows together in D -- is at most MIRROR_EPS_GATE decides.
        -> dict(desc, keep (as mirror_descriptor's, weights of 1), tau, eps, rows: with terms, truncated, out: compact_rows's) or
        None when no tau passes or none leaves a row out."""
        rows = np.asarray(rows, np.int64)
        drop = np.zeros(np.asarray(perm).shape[0], bool)
        drop[rows[dropped_rows]] = True
        drop[np.asarray(perm)[rows[dropped_rows]]] = True
        P = len(theta_twin)
        row_ptr, term_p = np.asarray(keep[0][0]), np.asarray(keep[1][0])
        for tau in RomEngine.MIRROR_COMPACT_TAUS:
            out = RomEngine.compact_rows(desc, keep, tau)
            kept = out["keep"] != 0
            if kept.all():
                continue
            eps = RomEngine.mirror_probe_eps(tables, perm, theta_twin, nprobe=RomEngine.MIRROR_PROBES, drop=drop,
                                             rotated=RomEngine.compact_tables(desc, keep, out, P))[0]
            if eps <= RomEngine.MIRROR_EPS_GATE:
                sel = np.repeat(kept, np.diff(row_ptr))
                new_ptr = np.concatenate([[0], np.cumsum(np.diff(row_ptr) * kept)])
                k = [i32(new_ptr), i32(term_p[sel]), f64(out["tv"][sel]), f64(out["rhs"]), keep[4], f64(np.ones(desc.n)), keep[6]]
                d = RomDesc(n=desc.n, r=desc.r, P=desc.P, n_obs=0, nterms=int(sel.sum()), row_ptr=k[0][1], term_p=k[1][1],
                            term_val=k[2][1], rhs=k[3][1], obs_phi=None)
                return {"desc": d, "keep": k, "tau": tau, "eps": eps, "rows": int(np.count_nonzero(np.diff(new_ptr))),
                        "truncated": int((~kept).sum()), "out": out}
        return None

    @staticmethod
    def mirror_form(r, P, tables, rhs, perm, rows, weight, theta_twin):
        """Host only.  The half form of one reduced model, gated: (b) r <= 80 (the grouped one-wave kernel), (c) the probes' eps at
        most MIRROR_EPS_GATE, (d) FINROM_ROM_NO_MIRROR not set; (a), the operator's own symmetry, is the caller's test
        (FomEngine.mirror_rows with col_twin).  A form that installs also gets a SHORT descriptor without the rows mirror_skip_rows
        selects, under the same gate (FINROM_ROM_KEEP_ROWS=1: none); the gate's probes lie in MIRROR_PROBE_RANGE, so only samples
        inside that range walk the short list, every other mirror-symmetric sample the half list with all rows.
        -> dict(eps: the gated value with the dropped rows counted, eps_all_rows: without them, dropped: their number, dropped_rows,
        tau, dropped_max: the largest dropped row's size relative to the largest row, installs, and when it installs: desc, keep,
        with dropped rows also desc_short, keep_short, and where mirror_compact_rows finds a threshold that passes the gate
        desc_compact, keep_compact, tau_compact, eps_compact, compact_rows, compact_truncated, compact_out; FINROM_ROM_NO_COMPACT=1:
        none of these) or None ((b) / (d))."""
        if _os.environ.get("FINROM_ROM_NO_MIRROR") is not None or r > 80:
            return None
        eps, Ts = RomEngine.mirror_probe_eps(tables, perm, theta_twin, nprobe=RomEngine.MIRROR_PROBES)
        form = {"eps": eps, "eps_all_rows": eps, "installs": bool(eps <= RomEngine.MIRROR_EPS_GATE), "Ts": Ts,
                "dropped": 0, "dropped_rows": np.zeros(len(rows), bool), "tau": None, "dropped_max": 0.0}
        if form["installs"]:
            if _os.environ.get("FINROM_ROM_KEEP_ROWS") is None:
                dropped, eps_c, tau, largest = RomEngine.mirror_skip_rows(tables, Ts, rhs, perm, rows, theta_twin)
                if eps_c is not None:
                    form.update(eps=eps_c, dropped=int(dropped.sum()), dropped_rows=dropped, tau=tau, dropped_max=largest)
            n = np.asarray(perm).shape[0]
            form["desc"], form["keep"] = RomEngine.mirror_descriptor(n, r, P, Ts, rows, weight, theta_twin, rhs)
            if form["dropped"]:
                form["desc_short"], form["keep_short"] = RomEngine.mirror_descriptor(n, r, P, Ts, rows, weight, theta_twin, rhs,
                                                                                 form["dropped_rows"])
                # ... and a COMPACT descriptor, the short one's rows rotated per pattern class (FINROM_ROM_NO_COMPACT=1: none)
                if _os.environ.get("FINROM_ROM_NO_COMPACT") is None:
                    c = RomEngine.mirror_compact_rows(tables, perm, theta_twin, rows, form["dropped_rows"], form["desc_short"],
                                                      form["keep_short"])
                    if c is not None:
                        form.update(desc_compact=c["desc"], keep_compact=c["keep"], tau_compact=c["tau"], eps_compact=c["eps"],
                                    compact_rows=c["rows"], compact_truncated=c["truncated"], compact_out=c["out"])
        return form

    def set_mirror(self, form):
        """Install a form of mirror_form (finrom_rom_set_mirror); the measured eps stays on the engine (mirror_eps) either way.
        -> installed?"""
        if form is None:
            return False
        self.mirror_eps = form["eps"]
        self.mirror_eps_all_rows = form["eps_all_rows"]
        if not form["installs"]:
            return False
        keep = form["keep"]
        rc = lib().finrom_rom_set_mirror(self._h, C.byref(form["desc"]), keep[4][1], keep[5][1], keep[6][1])
        if rc == _ffi.ERR_UNSUPPORTED:                    # no grouped form on this handle
            return False
        check(rc, "finrom_rom_set_mirror")
        self.mirror = True
        if "desc_short" in form:                          # in-range samples walk the list without the dropped rows
            lo, hi = self.MIRROR_PROBE_RANGE
            rc = lib().finrom_rom_set_mirror_short(self._h, C.byref(form["desc_short"]), form["keep_short"][5][1],
                                                   lo * (1.0 - 1e-12), hi * (1.0 + 1e-12))
            if rc != _ffi.ERR_UNSUPPORTED:                # (no grouped form for the short descriptor: the half list serves everybody)
                check(rc, "finrom_rom_set_mirror_short")
                self.mirror_dropped = form["dropped"]
                self.mirror_dropped_max = form["dropped_max"]
                if "desc_compact" in form:                # ... and the launches that offer it, the rotated rows (DESIGN 4b'')
                    rc = lib().finrom_rom_set_mirror_compact(self._h, C.byref(form["desc_compact"]), form["keep_compact"][5][1])
                    if rc != _ffi.ERR_UNSUPPORTED:
                        check(rc, "finrom_rom_set_mirror_compact")
                        self.mirror_eps_compact = form["eps_compact"]
        return True

    def mirror_info(self, short=None, compact=False):
        """(rows with terms, k-steps, k-steps with vector arithmetic) of a list on the handle as the native builder counts them
        (finrom_rom_mirror_info): short=True the short list, False the half list with all rows, None the one in-range samples
        walk (the short list if installed, else the half list); compact=True: the compact list; zeros where none is installed."""
        def get(which):
            o = [C.c_int32() for _ in range(3)]
            check(lib().finrom_rom_mirror_info(self._h, which, *[C.byref(x) for x in o]), "finrom_rom_mirror_info")
            return tuple(x.value for x in o)
        if compact:
            return get(2)
        if short is None:
            s = get(1)
            return s if s[1] else get(0)
        return get(1 if short else 0)

    def last_form(self):
        """'half' when the most recent projection launch of solve / solve_pairs offered its samples the half list (each sample
        whose parameters equal their twins' walked it), 'full' otherwise -- after every projection launch of grad as well, which never
        offers the half list --, 'none' before the first call (finrom_rom_last_form)."""
        rc = lib().finrom_rom_last_form(self._h)
        if rc < 0:
            check(rc, "finrom_rom_last_form")
        return _ffi.ROM_FORMS[rc]

    def last_epilogue(self):
        """'roomy' when the most recent projection launch ran the 256-register one-wave kernel (the pair path beside the FOM's half
        sweep, QoI-only, r <= 80) with a fixed wait behind every round of its epilogue's dependent MFMAs, 'roomy-short-waits' when
        it ran that kernel's form without the waits between accumulate-chained MFMAs (same bits; the pair path beside a sweep on
        its CU-masked stream, batches of 16 384 and more), 'roomy-block-row' when it ran the short-waits form that eliminates each
        block row in place instead of forming its diagonal tile's inverse (qoi_r differs at rounding level; there, at r = 65 .. 80),
        'standard' for every other kernel, 'none' before the first call
        (finrom_rom_last_epilogue)."""
        rc = lib().finrom_rom_last_epilogue(self._h)
        if rc < 0:
            check(rc, "finrom_rom_last_epilogue")
        return _ffi.ROM_EPILOGUES[rc]

    def solve(self, theta, want_state=False, want_w=True):
        """want_w=False: only the reduced QoI comes back; bases wider than 96 then factor and solve inside the projection
        kernel's registers (no A_r in memory)."""
        b = _Batch(theta, self.P)
        S, r = b.S, self.r
        w_r, wp = b.new((S, r)) if want_w else (None, None)
        qoi, qp = b.new((S, self.n_obs))
        info, ip = b.new((S,), "i4")
        A_r, Ap = (b.new((S, r, r)) if want_state else (None, None))
        B_r, Bp = (b.new((S, r)) if want_state else (None, None))
        check(lib().finrom_rom_solve(self._h, b.ptr, S, wp, qp, Ap, Bp, ip, b.stream), "finrom_rom_solve")
        out = {"qoi_r": b.out(qoi, (S, self.n_obs)), "info": b.out(info, (S,), "i4")}
        if want_w:
            out["w_r"] = b.out(w_r, (S, r))
        if want_state:
            out["A_r"] = b.out(A_r, (S, r, r)); out["B_r"] = b.out(B_r, (S, r))
        return out

    def set_gradient_blocks(self, pairs, G):
        """pairs: list of (p, i); G [npairs, r, r] with G[t] = (A_p Phi)^T (A_i Phi)  (finrom_rom_set_gradient)."""
        pp, pi = i32([p for p, _ in pairs]), i32([i for _, i in pairs])
        Gt = np.ascontiguousarray(np.transpose(np.asarray(G, dtype=np.float64), (0, 2, 1)))   # column by column
        check(lib().finrom_rom_set_gradient(self._h, len(pairs), pp[1], pi[1], Gt.ctypes.data_as(_ffi.c_f64p)),
              "finrom_rom_set_gradient")
        self._has_grad = True

    def set_gram_blocks(self, pairs, G):
        """pairs: list of (p, q), 0 <= p <= q <= P; G [npairs, r, r] symmetric blocks Psi_p^T Psi_q (+ transpose for p != q)
        (finrom_rom_set_gram)."""
        pp, pq = i32([p for p, _ in pairs]), i32([q for _, q in pairs])
        G = np.ascontiguousarray(G, dtype=np.float64)
        check(lib().finrom_rom_set_gram(self._h, len(pairs), pp[1], pq[1], G.ctypes.data_as(_ffi.c_f64p)), "finrom_rom_set_gram")
        self.gram_pairs = len(pairs)

    def set_projection(self, mode):
        """'direct' (per-sample psi^T psi on MFMA, the reference's contraction) or 'offline_online' (precomputed blocks)."""
        code = {"direct": 0, "offline_online": 1}[mode]
        check(lib().finrom_rom_set_projection(self._h, code), "finrom_rom_set_projection")
        self.projection = mode

    def grad(self, theta, data):
        """theta [S, P], data [n_obs] or [S, n_obs] -> dict(J [S], g [S, P], w_r, qoi_r, info)."""
        b = _Batch(theta, self.P)
        S = b.S
        data = np.ascontiguousarray(data, dtype=np.float64) if not _is_torch(data) else data
        per_sample = 1 if data.ndim == 2 else 0
        db = _Batch(data, self.n_obs)
        J, Jp = b.new((S,)); g, gp = b.new((S, self.P)); w_r, wp = b.new((S, self.r))
        qoi, qp = b.new((S, self.n_obs)); info, ip = b.new((S,), "i4")
        check(lib().finrom_rom_grad(self._h, b.ptr, db.ptr, per_sample, S, Jp, gp, wp, qp, ip, b.stream), "finrom_rom_grad")
        _sync_if_mixed(b, db)
        return {"J": b.out(J, (S,)), "g": b.out(g, (S, self.P)), "w_r": b.out(w_r, (S, self.r)),
                "qoi_r": b.out(qoi, (S, self.n_obs)), "info": b.out(info, (S,), "i4")}

    def close(self):
        if getattr(self, "_h", None):
            _ffi.destroy_handle("finrom_rom_destroy", self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class SubfinAverager:
    """theta = S k on the device (finrom_subfin_avg)."""

    def __init__(self, Sop):
        Sop = np.ascontiguousarray(Sop, dtype=np.float64)
        self.P, self.n = Sop.shape
        self._S = DeviceBuffer.from_numpy(Sop)

    def __call__(self, K):
        b = _Batch(K, self.n)
        th, tp = b.new((b.S, self.P))
        check(lib().finrom_subfin_avg(self._S.ptr, self.P, self.n, b.ptr, b.S, tp, b.stream), "finrom_subfin_avg")
        self._S.used_on(b.stream)
        return b.out(th, (b.S, self.P))

    def on_device(self, K):
        """NumPy K [S, n] -> theta as a DeviceArray (no copy back): the next library call consumes it in place."""
        b = _Batch(K, self.n)
        buf = DeviceBuffer(max(b.S * self.P * 8, 8))
        check(lib().finrom_subfin_avg(self._S.ptr, self.P, self.n, b.ptr, b.S, buf.ptr, None), "finrom_subfin_avg")
        out = DeviceArray(buf, (b.S, self.P))
        out._src = b.keep                                  # (the input's staging buffer lives until theta has been consumed)
        return out


class FieldSampler:
    """k = exp(0.5 * xi @ U) on the device (finrom_sampler_*)."""

    def __init__(self, U):
        U = np.ascontiguousarray(U, dtype=np.float64)
        self.n = U.shape[0]
        h = C.c_void_p()
        check(lib().finrom_sampler_create(U.ctypes.data_as(_ffi.c_f64p), self.n, C.byref(h)), "finrom_sampler_create")
        self._h = h

    def __call__(self, xi):
        b = _Batch(xi, self.n)
        k, kp = b.new((b.S, self.n))
        check(lib().finrom_sampler_draw(self._h, b.ptr, b.S, kp, b.stream), "finrom_sampler_draw")
        return b.out(k, (b.S, self.n))

    def field(self, v, mean=None):
        """k = mean + v @ U row-wise (finrom_sampler_field): the latent Gaussian field of the whitened variable v [S, n] without
        the exp of __call__.  mean: [n] or None (zero).  NumPy in -> NumPy out; a float64 CUDA tensor in -> a tensor on its device,
        launched on torch's current stream (mean then a tensor on that device, or anything torch.as_tensor takes)."""
        b = _Batch(v, self.n)
        mp, mb = None, None
        if mean is not None:
            if b.torch:
                import torch
                mean = torch.as_tensor(mean, dtype=torch.float64, device=b.device)
            elif _is_torch(mean):
                mean = mean.detach().cpu().numpy()
            mb = _Batch(mean, self.n)
            if mb.S != 1:
                raise ValueError("field: mean must be one field of %d values" % self.n)
            mp = mb.ptr
        k, kp = b.new((b.S, self.n), zero=False)
        check(lib().finrom_sampler_field(self._h, mp, b.ptr, b.S, kp, b.stream), "finrom_sampler_field")
        return b.out(k, (b.S, self.n))

    def pullback(self, g):
        """U g row-wise (finrom_sampler_pullback): the gradient g [S, n] of a function of the field as a gradient in v."""
        b = _Batch(g, self.n)
        out, op = b.new((b.S, self.n), zero=False)
        check(lib().finrom_sampler_pullback(self._h, b.ptr, b.S, op, b.stream), "finrom_sampler_pullback")
        return b.out(out, (b.S, self.n))

    def draw(self, seed, first, S, like=None, want_xi=False):
        """S fields of the stream `seed` starting at GLOBAL sample index `first`, xi drawn on the device (Philox keyed by the
        global index: independent of how a dataset is sharded).  like: a torch CUDA tensor (-> torch outputs on its device /
        current stream) or None (-> NumPy).  Returns k [S, n] (and xi [S, n] if want_xi)."""
        b = _Batch(like if like is not None else np.zeros((0, self.n)), self.n)
        k, kp = b.new((S, self.n))
        xi, xp = b.new((S, self.n)) if want_xi else (None, None)
        check(lib().finrom_sampler_draw_seeded(self._h, int(seed), int(first), int(S), kp, xp, b.stream), "finrom_sampler_draw_seeded")
        out = b.out(k, (S, self.n))
        return (out, b.out(xi, (S, self.n))) if want_xi else out

    def close(self):
        if getattr(self, "_h", None):
            _ffi.destroy_handle("finrom_sampler_destroy", self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class MetricHandle:
    """The low-rank metric M = I + V diag(lam) V^T on the device (finrom_metric_*): Vt [rho, n] orthonormal rows, lam [rho] > 0,
    1 <= rho <= 64.  apply(x, op): y = x + sum_j c_j V_j (V_j . x) row-wise for op in 'M', 'inv', 'sqrt', 'invsqrt'.  NumPy in ->
    NumPy out; a float64 CUDA tensor in -> a tensor on its device, launched on torch's current stream."""
    OPS = {"M": 0, "inv": 1, "sqrt": 2, "invsqrt": 3}

    def __init__(self, Vt, lam):
        Vt = np.ascontiguousarray(Vt, dtype=np.float64)
        lam = np.ascontiguousarray(lam, dtype=np.float64)
        if Vt.ndim != 2 or lam.shape != (Vt.shape[0],):
            raise ValueError("MetricHandle: Vt [rho, n] and lam [rho]")
        self.rho, self.n = Vt.shape
        h = C.c_void_p()
        check(lib().finrom_metric_create(Vt.ctypes.data_as(_ffi.c_f64p), lam.ctypes.data_as(_ffi.c_f64p), self.n, self.rho, C.byref(h)),
              "finrom_metric_create")
        self._h = h

    def apply(self, x, op="M", want_quad=False):
        """y [S, n] (and quad [S] = x . y row-wise if want_quad)."""
        b = _Batch(x, self.n)
        y, yp = b.new((b.S, self.n), zero=False)
        q, qp = b.new((b.S,), zero=False) if want_quad else (None, None)
        check(lib().finrom_metric_apply(self._h, self.OPS[op], b.ptr, b.S, yp, qp, b.stream), "finrom_metric_apply")
        out = b.out(y, (b.S, self.n))
        return (out, b.out(q, (b.S,))) if want_quad else out

    def close(self):
        if getattr(self, "_h", None):
            _ffi.destroy_handle("finrom_metric_destroy", self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class DeviceErrorModel:
    """The learned error model on the device (finrom_mlp_*): the weights of a deep_learning/dl_model.py::ResBnFcModel (the
    stand-in for the reference's Keras res_bn_fc_model, dl_model.py:149-176), batch normalisation folded into scale / shift in
    fp32 exactly as the host model does."""

    @staticmethod
    def fold(model):
        """The fp32 arrays of finrom_mlp_desc for a ResBnFcModel: scale = gamma / sqrt(var + eps) and shift = beta - mean scale
        formed in fp32 (what the device evaluates; tests/mlp_cases.py widens these same arrays for its float64 reference)."""
        from .deep_learning.dl_model import BN_EPS
        layers = list(model.units) + [model.head]
        f32 = lambda a_: np.ascontiguousarray(a_, dtype=np.float32)
        scale = np.stack([u["gamma"] / np.sqrt(u["var"] + np.float32(BN_EPS)) for u in layers]).astype(np.float32)
        shift = np.stack([u["beta"] - u["mean"] * s_ for u, s_ in zip(layers, scale)]).astype(np.float32)
        L, nw = len(model.units), model.n_weights
        return {"W0": f32(model.W0), "b0": f32(model.b0), "scale": f32(scale), "shift": f32(shift),
                "W": f32(np.stack([u["W"] for u in model.units]) if L else np.zeros((0, nw, nw))),
                "b": f32(np.stack([u["b"] for u in model.units]) if L else np.zeros((0, nw))),
                "Wh": f32(model.head["W"]), "bh": f32(model.head["b"])}

    def __init__(self, model):
        arrs = self.fold(model)
        L, nw = len(model.units), model.n_weights
        self.n_in, self.n_out = model.n_in, model.n_out
        d = MlpDesc(n_in=model.n_in, n_w=nw, n_layers=L, n_out=model.n_out,
                    **{k: v.ctypes.data_as(_ffi.c_f32p) for k, v in arrs.items()})
        h = C.c_void_p()
        check(lib().finrom_mlp_create(C.byref(d), C.byref(h)), "finrom_mlp_create")
        self._h = h

    def predict(self, K):
        b = _Batch(K, self.n_in)
        e, ep = b.new((b.S, self.n_out))
        check(lib().finrom_mlp_predict(self._h, b.ptr, b.S, ep, b.stream), "finrom_mlp_predict")
        return b.out(e, (b.S, self.n_out))

    def misfit_grad(self, K, data, want_grad=True):
        """finrom_mlp_misfit_grad: the network as a model of its own (the reference's pure deep-learning surrogate) for a batch of
        nodal fields K [S, n]: out = NN(K), loss = 1/2 |data - out|^2, grad = -vjp(data - out).  data [n_out] or [S, n_out], or
        None (prediction only: loss and grad are None).  NumPy in, NumPy out; torch in, torch out on the current stream.
        -> dict(loss [S], grad [S, n] or None, out [S, n_out])."""
        n, no = self.n_in, self.n_out
        b = _Batch(K, n)
        S = b.S
        out, op = b.new((S, no), zero=False)
        if data is None:
            if want_grad:
                raise ValueError("misfit_grad: the gradient needs data")
            check(lib().finrom_mlp_misfit_grad(self._h, b.ptr, None, 0, S, None, None, op, b.stream), "finrom_mlp_misfit_grad")
            return {"loss": None, "grad": None, "out": b.out(out, (S, no))}
        data = data if _is_torch(data) else np.ascontiguousarray(data, dtype=np.float64)
        if data.shape[-1] != no or (data.ndim == 2 and data.shape[0] != S) or data.ndim > 2:
            raise ValueError(f"misfit_grad: data must be [{no}] or [{S}, {no}], got {tuple(data.shape)}")
        per_sample = 1 if data.ndim == 2 else 0
        db = _Batch(data, no)
        loss, lp = b.new((S,), zero=False)
        grad, gp = b.new((S, n), zero=False) if want_grad else (None, None)
        check(lib().finrom_mlp_misfit_grad(self._h, b.ptr, db.ptr, per_sample, S, gp, lp, op, b.stream), "finrom_mlp_misfit_grad")
        _sync_if_mixed(b, db)
        return {"loss": b.out(loss, (S,)), "grad": b.out(grad, (S, n)) if want_grad else None, "out": b.out(out, (S, no))}

    def set_tile_min(self, tile_min):
        """Batches of at least tile_min samples take misfit_grad's tile form (default 4096)."""
        check(lib().finrom_mlp_set_tile_min(self._h, int(tile_min)), "finrom_mlp_set_tile_min")

    def last_form(self):
        """The form the last misfit_grad took: 0 none yet, 1 per-sample, 2 tile."""
        return int(lib().finrom_mlp_last_form(self._h))

    def close(self):
        if getattr(self, "_h", None):
            _ffi.destroy_handle("finrom_mlp_destroy", self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class DeviceTrainer:
    """Training of the learned error model on the device (finrom_mlp_train_*, csrc/mlp_train.hip): the handle owns parameters,
    Adam's state, moving statistics, tape and workspaces; the dataset stays resident as fp32 torch tensors; an epoch's steps are
    captured once in a HIP graph and replayed (a linear chain of library launches on one stream; each step takes its rows by
    index from the epoch's permutation, uploaded into the same device buffer before each replay).  The host statement is
    ResBnFcModel.fit_host; ResBnFcModel.fit is the front door."""

    def __init__(self, model, max_batch=500):
        self.model = model
        d = _ffi.MlpTrainDesc(n_in=model.n_in, n_w=model.n_weights, n_layers=model.n_layers, n_out=model.n_out, max_batch=int(max_batch))
        h = C.c_void_p()
        check(lib().finrom_mlp_train_create(C.byref(d), C.byref(h)), "finrom_mlp_train_create")
        self._h = h
        self.max_batch = int(max_batch)
        self.n_flat = int(lib().finrom_mlp_train_param_count(h))
        self.push()

    @staticmethod
    def _stream():
        import torch
        return torch.cuda.current_stream().cuda_stream

    # -- state to and from the host model ------------------------------------------------------------------------------------------
    def push(self):
        """The model's parameters, moving statistics and optimiser state -> the handle."""
        m = self.model
        fp = lambda a_: a_.ctypes.data_as(_ffi.c_f32p)
        p = m.flatten(m._tree())
        assert p.size == self.n_flat
        mm = m.flatten(m.opt["m"]) if m.opt["m"] is not None else None
        vv = m.flatten(m.opt["v"]) if m.opt["v"] is not None else None
        check(lib().finrom_mlp_train_set_params(self._h, fp(p), fp(mm) if mm is not None else None, fp(vv) if vv is not None else None,
                                                int(m.opt["t"])), "finrom_mlp_train_set_params")

    def pull(self):
        """The handle's parameters, moving statistics, m, v, t -> the model (fp32 arrays)."""
        m = self.model
        p, mm, vv = (np.empty(self.n_flat, np.float32) for _ in range(3))
        t = C.c_int64()
        fp = lambda a_: a_.ctypes.data_as(_ffi.c_f32p)
        check(lib().finrom_mlp_train_get_params(self._h, fp(p), fp(mm), fp(vv), C.byref(t)), "finrom_mlp_train_get_params")
        m.set_tree(m.unflatten(p))
        m.opt["m"], m.opt["v"], m.opt["t"] = m.unflatten(mm), m.unflatten(vv), int(t.value)

    def get_grads(self):
        """-> (loss, MAPE, gradient tree with the batch statistics in "mean" / "var") of the last finrom_mlp_train_grad."""
        g = np.empty(self.n_flat, np.float32); lm = np.empty(2)
        check(lib().finrom_mlp_train_get_grads(self._h, g.ctypes.data_as(_ffi.c_f32p), lm.ctypes.data_as(_ffi.c_f64p)), "finrom_mlp_train_get_grads")
        return float(lm[0]), float(lm[1]), self.model.unflatten(g)

    def set_grads(self, grads, loss=0.0, mape=0.0, B=2):
        g = self.model.flatten(grads); lm = np.array([loss, mape], dtype=np.float64)
        check(lib().finrom_mlp_train_set_grads(self._h, g.ctypes.data_as(_ffi.c_f32p), lm.ctypes.data_as(_ffi.c_f64p), int(B)), "finrom_mlp_train_set_grads")

    # -- the calls -----------------------------------------------------------------------------------------------------------------
    def set_lr(self, lr):
        check(lib().finrom_mlp_train_set_lr(self._h, float(lr), self._stream()), "finrom_mlp_train_set_lr")

    def grad(self, X, Y, rows):
        """X [S, n_in], Y [S, n_out] fp32 and rows [B] int32: contiguous CUDA tensors."""
        check(lib().finrom_mlp_train_grad(self._h, X.data_ptr(), Y.data_ptr(), rows.data_ptr(), int(rows.numel()), self._stream()), "finrom_mlp_train_grad")

    def apply(self):
        check(lib().finrom_mlp_train_apply(self._h, self._stream()), "finrom_mlp_train_apply")

    def epoch_stats(self, reset=True):
        """-> (row-weighted mean loss, mean MAPE, rows) of the steps since the last reset; .last_mse: the mean loss without the
        regulariser."""
        o = np.zeros(4)
        check(lib().finrom_mlp_train_epoch_stats(self._h, o.ctypes.data_as(_ffi.c_f64p), 1 if reset else 0, self._stream()), "finrom_mlp_train_epoch_stats")
        self.last_mse = o[3] / o[2] if o[2] > 0 else 0.0
        return (o[0] / o[2], o[1] / o[2], int(o[2])) if o[2] > 0 else (0.0, 0.0, 0)

    def evaluate(self, X, Y):
        """Inference form over CUDA fp32 tensors -> (loss with the regulariser, MAPE)."""
        o = np.zeros(2)
        check(lib().finrom_mlp_train_eval(self._h, X.data_ptr(), Y.data_ptr(), int(X.shape[0]), o.ctypes.data_as(_ffi.c_f64p), self._stream()), "finrom_mlp_train_eval")
        return float(o[0]), float(o[1])

    def export(self):
        """The trained weights as a DeviceErrorModel (finrom_mlp_predict / finrom_romml_grad), through the host model's arrays."""
        self.pull()
        return DeviceErrorModel(self.model)

    @staticmethod
    def to_device(a, n):
        import torch
        return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.float32).reshape(-1, n))).cuda()

    def fit(self, z, errors, *, epochs, batch_size=500, shuffle=True, validation_data=None, lr=3e-4, seed=0, graph=True, record_steps=False):
        """ResBnFcModel.fit_host's run on the device: the same permutations (EpochPlan), the same history object.
        record_steps: read every step's loss back (history.step_loss; stream order, one synchronisation per step)."""
        import torch
        from .deep_learning.dl_model import EpochPlan, History
        m = self.model
        X, Y = self.to_device(z, m.n_in), self.to_device(errors, m.n_out)
        plan = EpochPlan(X.shape[0], batch_size, shuffle, seed, m.opt["epoch"])
        if plan.B > self.max_batch:
            raise ValueError(f"DeviceTrainer.fit: batch of {plan.B} rows exceeds max_batch = {self.max_batch}")
        val = None if validation_data is None else (self.to_device(validation_data[0], m.n_in), self.to_device(validation_data[1], m.n_out))
        rows_dev = torch.zeros(plan.S, dtype=torch.int32, device="cuda")
        slices = [rows_dev[i:i + plan.B] for i in range(0, plan.S, plan.B)]
        self.push()
        hist = History(val is not None)

        def epoch(record=False):
            for r in slices:
                self.grad(X, Y, r)
                if record:
                    hist.step_loss.append(self.get_grads()[0])
                self.apply()
        g = None
        if graph and not record_steps and epochs > 0:
            try:
                side = torch.cuda.Stream()
                side.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(side):                           # warm-up on a side stream, as torch's graph recipe asks:
                    self.set_lr(0.0)                                    # one step on valid rows, then the state is put back
                    self.grad(X, Y, slices[0]); self.apply()
                torch.cuda.current_stream().wait_stream(side)
                torch.cuda.synchronize()
                self.push(); self.epoch_stats(reset=True)
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g):
                    epoch()
            except _ffi.FinromError:                                    # the library's own error is an error, graph or not
                raise
            except RuntimeError as exc:                                 # torch could not capture this sequence: plain stream order
                import warnings
                warnings.warn(f"DeviceTrainer: HIP graph capture failed ({exc!r}); the steps are launched kernel by kernel")
                g = None
                self.push(); self.epoch_stats(reset=True)
        self.graph_used = g is not None
        for _ in range(int(epochs)):
            e = m.opt["epoch"]
            self.set_lr(lr(e) if callable(lr) else lr)
            rows = plan.next_rows()
            if rows.min() < 0 or rows.max() >= plan.S:
                raise ValueError("DeviceTrainer.fit: row index outside [0, S)")
            rows_dev.copy_(torch.from_numpy(np.ascontiguousarray(rows, dtype=np.int32)))
            if g is not None:
                g.replay()
            else:
                epoch(record_steps)
            loss, mape, _ = self.epoch_stats(reset=True)
            hist.mse.append(self.last_mse)
            m.opt["epoch"] = e + 1
            hist.add(loss, mape, self.evaluate(*val) if val is not None else None)
        torch.cuda.synchronize()
        self.pull()
        return hist

    def close(self):
        if getattr(self, "_h", None):
            _ffi.destroy_handle("finrom_mlp_train_destroy", self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def romml_grad(rom, mlp, Sop_buf, K, data):
    """finrom_romml_grad: value and gradient of the ROM + learned-error misfit for a batch of nodal fields K [S, n] in ONE
    library call (sub-fin averages, network forward, ROM adjoint against data - e_NN, network backward + chain rule).
    -> dict(grad [S, n], loss [S], qoi_r, e_NN, info)."""
    n, n_obs = mlp.n_in, mlp.n_out
    b = _Batch(K, n)
    S = b.S
    data = data if _is_torch(data) else np.ascontiguousarray(data, dtype=np.float64)
    per_sample = 1 if data.ndim == 2 else 0
    db = _Batch(data, n_obs)
    grad, gp = b.new((S, n), zero=False); loss, lp = b.new((S,), zero=False); q, qp = b.new((S, n_obs), zero=False)
    e, ep = b.new((S, n_obs), zero=False); info, ip = b.new((S,), "i4", zero=False)      # (finrom_romml_grad overwrites info)
    check(lib().finrom_romml_grad(rom._h, mlp._h, Sop_buf.ptr, b.ptr, db.ptr, per_sample, S, gp, lp, qp, ep, ip, b.stream),
          "finrom_romml_grad")
    Sop_buf.used_on(b.stream)
    _sync_if_mixed(b, db)
    return {"grad": b.out(grad, (S, n)), "loss": b.out(loss, (S,)), "qoi_r": b.out(q, (S, n_obs)), "e_NN": b.out(e, (S, n_obs)),
            "info": b.out(info, (S,), "i4")}


def device_sub(a, b_):
    """a - b elementwise on the device (generate_fin_dataset.py:99)."""
    ba = _Batch(a, 1)
    bb = _Batch(b_, 1)
    out, op = ba.new((ba.S,))
    check(lib().finrom_sub(ba.ptr, bb.ptr, ba.S, op, ba.stream), "finrom_sub")
    res = ba.out(out, (ba.S,))
    return res.reshape(a.shape)
