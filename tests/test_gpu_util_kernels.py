"""The helper kernels at the head of both workloads (csrc/util_kernels.hip), each against a plain reference at its size classes and
branches: the Gaussian-field sampler's 64 x 64 kernel and its blocked GEMM kernel in three forms (A, B), the three sub-fin average
kernels (C), the Philox normal kernel with the seeded draw's cut into pieces (D) and the difference kernel (E).

A and the first half of C use EXACT-SUM inputs: integers times a power of two, small enough that every product and every partial
sum in any order is exact in fp64.  The device's dot products then equal NumPy's bit for bit whatever the order, the tiling or the
use of FMA, and a misplaced, missing or doubled term shows at full size instead of at rounding level."""
import numpy as np
import pytest

from oracle import fin_oracle as O
from test_gpu_hmc_rng import GRID_CAP, PAD, SEEDS
from test_gpu_sampler import _factor

pytestmark = pytest.mark.gpu

U53 = 2.0 ** -53                     # fp64 unit roundoff
GRID = 2.0 ** -8                     # the exact-sum grid of U (A) and Sop (C)
NAN = float("nan")
FORMS = ("small", "gemm", "wm2", "nopad")


def _cuda(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.device("cuda", torch.cuda.current_device()))


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def _select(form, monkeypatch):
    """The environment of one sampler form: the 64 x 64 kernel, the GEMM kernel (256 x 128 tiles, padded lockstep), its 128 x 128
    instantiation, and the GEMM kernel with every tile stopping at its own K end."""
    for name in ("FINROM_SAMPLER_WM", "FINROM_SAMPLER_NO_PAD"):
        monkeypatch.delenv(name, raising=False)
    monkeypatch.setenv("FINROM_SAMPLER_GEMM_MIN", str(1 << 40) if form == "small" else "1")
    if form == "wm2":
        monkeypatch.setenv("FINROM_SAMPLER_WM", "2")
    if form == "nopad":
        monkeypatch.setenv("FINROM_SAMPLER_NO_PAD", "1")


def _forms(smp, xt, monkeypatch):
    out = {}
    for form in FORMS:
        _select(form, monkeypatch)
        out[form] = smp(xt).cpu().numpy()
    return out


def _draw_padded(smp, xi):
    """finrom_sampler_draw into a NaN-filled buffer PAD elements longer than the block (tests/test_gpu_hmc_rng.py::_draw): nothing
    behind the block may have changed, nothing inside may have stayed NaN."""
    import torch
    from bayesianinferencedl_amd import _ffi
    S, n = xi.shape
    xt = _cuda(xi)
    k = torch.full((S * n + PAD,), NAN, dtype=torch.float64, device=xt.device)
    _ffi.check(_ffi.lib().finrom_sampler_draw(smp._h, xt.data_ptr(), S, k.data_ptr(), _stream()), "finrom_sampler_draw")
    k = k.cpu().numpy()
    assert np.isnan(k[S * n:]).all(), "finrom_sampler_draw wrote behind its block"
    assert not np.isnan(k[:S * n]).any(), "finrom_sampler_draw left an element of its block unwritten"
    return k[:S * n].reshape(S, n)


# ---- A. sampler, exact-sum inputs, every element ---------------------------------------------------------------------------------
def _exact_inputs(n, S, seed):
    """xi: integers in [-7, 7]; U: upper triangular, integers in [-8, 8] (diagonal 1..8) times GRID = 2^-8.  Every product is an
    integer multiple of 2^-8 below 56, every partial sum of a column's n <= 4101 terms in ANY order one below 4101 x 56 < 2^18: all
    exact in fp64.  -> (xi, U, acc = xi @ U), acc checked here against the int64 product of the integers (all rows, or `some` rows
    where the int64 product of all of them would take minutes)."""
    rng = np.random.default_rng(seed)
    Ui = np.triu(rng.integers(-8, 9, (n, n)))
    Ui[np.arange(n), np.arange(n)] = rng.integers(1, 9, n)
    xii = rng.integers(-7, 8, (S, n))
    xi, U = xii.astype(np.float64), Ui * GRID
    acc = xi @ U
    rows = np.arange(S) if S * n * n <= 1 << 27 else np.unique(np.linspace(0, S - 1, 16).astype(int))
    assert np.array_equal(acc[rows], (xii[rows] @ Ui).astype(np.float64) * GRID), "the exact-sum inputs are not exact"
    assert int(np.abs(xii).max()) * int(np.abs(Ui).max()) * n < 1 << 53
    assert np.max(np.abs(0.5 * acc)) < 30.0, np.max(np.abs(0.5 * acc))
    return xi, U, acc


def _assert_forms(got, ref, what):
    for form in FORMS:
        err = np.max(np.abs(got[form] / ref - 1.0))
        assert err <= 1e-13, (what, form, err)
        assert np.array_equal(got[form], got["small"]), (what, form, "differs from the 64 x 64 kernel")


A_S = (1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025)


@pytest.mark.parametrize("n", [1, 7, 16, 17, 40, 64, 65, 80, 128, 129, 144, 256])
def test_sampler_exact_sums_every_element_in_four_forms(n, monkeypatch):
    """k = exp(0.5 xi U) with exact-sum inputs (_exact_inputs: xi in [-7, 7], U on the grid 2^-8 x [-8, 8]) in the 64 x 64 kernel, the
    GEMM kernel, its WM = 2 form and its NO_PAD form: the four bit-identical, each within 1e-13 relative (the bound of
    tests/test_gpu_sampler.py) of NumPy at EVERY element.  The sums being exact, only exp lies between device and NumPy, so 1e-13 is
    loose -- and still decisive: one unit of the grid in one term moves a field by 0.5 x 2^-8 = 1.95e-3 relative, a margin of 2e10.
    n = 1 .. 256: column tile 0 has nch = ceil(min(n, 128) / 16) = 1, 1, 1, 2, 3, 4, 5, 5, 8 K-chunks -- the prologue's gload(1) and
    gload(2), the two-chunk loop's odd tail and its `ch + 3 < nch` guard each taken and not taken; a last chunk with (n % 16 != 0) and
    without the k >= n select; wave column 1 with no live tile (n <= 64), one (n = 65, 80) and all (n = 128, 256); two column tiles.
    S = 1 .. 1025: slices of one input; one partial 64- / 256-row tile, full tiles, a second sample group of one row -- and row s of
    every batch is bitwise row s of the largest."""
    from bayesianinferencedl_amd.engine import FieldSampler
    xi, U, acc = _exact_inputs(n, max(A_S), 1000 + n)
    ref = np.exp(0.5 * acc)
    smp = FieldSampler(U)
    xt = _cuda(xi)
    whole = None
    for S in sorted(A_S, reverse=True):
        got = _forms(smp, xt[:S], monkeypatch)
        _assert_forms(got, ref[:S], (n, S))
        if whole is None:
            whole = got["small"]
        assert np.array_equal(got["small"], whole[:S]), (n, S, "rows depend on the batch")


@pytest.mark.parametrize("n,S", [(2050, 1100), (4101, 300)])
def test_sampler_padded_lockstep_exact_sums_every_element(n, S, monkeypatch):
    """The padded lockstep of sampler_gemm_kernel -- a column group runs to its top tile's K end when (top + 1) * 128 >= 2048, n >= 1921
    -- with the inputs, the four forms and the bounds of the test above, every element.  Here NO_PAD is another launch than the
    default, and its bit-equality is the claim "the padding adds exact zeros".
    n = 2050, S = 1100: padded top group (column tiles 9..16), unpadded group (1..8), the lone tile 0, 2 live columns in the last tile,
    a partial second sample group.  n = 4101, S = 300: the production mesh, five column groups of which three are padded."""
    from bayesianinferencedl_amd.engine import FieldSampler
    assert n >= 1921
    xi, U, acc = _exact_inputs(n, S, 1000 + n)
    got = _forms(FieldSampler(U), _cuda(xi), monkeypatch)
    _assert_forms(got, np.exp(0.5 * acc), (n, S))


@pytest.mark.parametrize("n,S", [(65, 65), (2050, 257)])
def test_sampler_writes_its_block_and_nothing_behind_it(n, S, monkeypatch):
    """finrom_sampler_draw through ctypes into NaN-filled buffers five elements longer than the block, all four forms: a last tile of
    one live column / two live columns and of one live row; the fields are those of NumPy besides."""
    from bayesianinferencedl_amd.engine import FieldSampler
    xi, U, acc = _exact_inputs(n, S, 2000 + n)
    smp = FieldSampler(U)
    got = {}
    for form in FORMS:
        _select(form, monkeypatch)
        got[form] = _draw_padded(smp, xi)
    _assert_forms(got, np.exp(0.5 * acc), (n, S))


# ---- B. sampler, real inputs, extended precision ---------------------------------------------------------------------------------
B_S = 300
B_ROWS = (0, 1, 63, 64, 100, 127, 128, 255, 256, 257, B_S - 2, B_S - 1)


@pytest.fixture(scope="module")
def real_case():
    """(U, xi) of section B per n, built once: U = tests/test_gpu_sampler.py::_factor(n, n), xi standard normal [300, n]."""
    cache = {}

    def get(n):
        if n not in cache:
            cache[n] = (_factor(n, n), np.random.default_rng(7 * n).standard_normal((B_S, n)))
        return cache[n]
    return get


@pytest.mark.parametrize("n", [40, 129, 2050, 4101])
def test_sampler_real_inputs_within_the_dot_product_bound_of_longdouble(n, real_case, monkeypatch):
    """U = _factor(n, n), xi standard normal, S = 300, the GEMM kernel and the 64 x 64 kernel against exp(0.5 xi U) in np.longdouble
    (64-bit mantissa); all rows below n = 2050, from there the twelve rows B_ROWS.  Per element
        |k / k_ref - 1| <= 0.5 (j + 1) u (|xi[s]| . |U[:, j]|) + 8 u,   u = 2^-53:
    the first-order worst case of a (j + 1)-term dot product in any order, with or without FMA (the padded terms are exact zeros),
    halved by the exponent's 0.5; 8 u for exp on both sides and the final rounding.  With term j // 2 of every column dropped, NumPy's
    fp64 product exceeds the bound at every checked element, by a factor of 7.6e3 at the least (n = 4101).
    Largest ratio to the bound measured on an MI355X, n = 40 / 129 / 2050 / 4101: 0.160 / 0.155 / 0.119 / 0.135 in both kernels (which
    are bit-identical); NumPy's own fp64 product with these inputs: 0.142 / 0.155 / 0.120 / 0.135."""
    from bayesianinferencedl_amd.engine import FieldSampler
    assert np.finfo(np.longdouble).eps <= 2.0 ** -63
    U, xi = real_case(n)
    rows = np.arange(B_S) if n < 2050 else np.array(B_ROWS)
    acc = xi[rows].astype(np.longdouble) @ U.astype(np.longdouble)
    ref = np.exp(0.5 * acc)
    bound = 0.5 * np.arange(1, n + 1) * U53 * (np.abs(xi[rows]) @ np.abs(U)) + 8 * U53
    smp = FieldSampler(U)
    xt = _cuda(xi)
    worst = {}
    for form in ("gemm", "small"):
        _select(form, monkeypatch)
        k = smp(xt).cpu().numpy()
        ratio = (np.abs(k[rows].astype(np.longdouble) / ref - 1) / bound).astype(np.float64)
        worst[form] = float(np.max(ratio))
        print("sampler n = %d %s: largest |k / k_ref - 1| / bound = %.3f" % (n, form, worst[form]))
    host = np.exp(0.5 * (xi[rows] @ U))
    print("sampler n = %d NumPy fp64: %.3f" % (n, float(np.max((np.abs(host.astype(np.longdouble) / ref - 1) / bound).astype(np.float64)))))
    for form, w in worst.items():
        assert w <= 1.0, (n, form, w)


@pytest.mark.parametrize("n", [129, 2050])
def test_sampler_nan_rows_stay_in_their_rows(n, real_case, monkeypatch):
    """Rows 1, 104 (the middle of a 16-row MFMA tile and of a 64-row wave tile) and S - 1 of xi set to NaN, all four forms: those rows
    come back all NaN, every other row is bit-identical to the clean run.  n % 16 != 0 at both sizes: the last K-chunk of row s reads
    the head of row s + 1 and must select it away, not multiply it by zero."""
    from bayesianinferencedl_amd.engine import FieldSampler
    U, xi = real_case(n)
    bad = np.array([1, 104, B_S - 1])
    good = np.setdiff1d(np.arange(B_S), bad)
    xn = xi.copy()
    xn[bad] = NAN
    smp = FieldSampler(U)
    clean = _forms(smp, _cuda(xi), monkeypatch)
    dirty = _forms(smp, _cuda(xn), monkeypatch)
    for form in FORMS:
        assert not np.isnan(clean[form]).any(), (n, form)
        assert np.isnan(dirty[form][bad]).all(), (n, form, "a NaN row came back with finite fields")
        assert np.array_equal(dirty[form][good], clean[form][good]), (n, form, "a NaN row changed another row")


# ---- C. sub-fin averages ---------------------------------------------------------------------------------------------------------
def _avg_padded(avg, K):
    """finrom_subfin_avg into a NaN-filled buffer PAD elements longer than S * P."""
    import torch
    from bayesianinferencedl_amd import _ffi
    S = K.shape[0]
    kt = _cuda(K)
    th = torch.full((S * avg.P + PAD,), NAN, dtype=torch.float64, device=kt.device)
    _ffi.check(_ffi.lib().finrom_subfin_avg(avg._S.ptr, avg.P, avg.n, kt.data_ptr(), S, th.data_ptr(), _stream()), "finrom_subfin_avg")
    th = th.cpu().numpy()
    assert np.isnan(th[S * avg.P:]).all(), "finrom_subfin_avg wrote behind S * P"
    return th[:S * avg.P].reshape(S, avg.P)


C_EXACT = ([("small", P, n, (1, 255, 256, 257)) for P in (1, 5, 9, 16) for n in (1, 5, 9, 16)]
           + [("10x4", P, n, (1, 2, 3, 4, 5, 17)) for P in (1, 9, 10) for n in (17, 64, 255, 256, 257, 1597)]
           + [("16x2", P, n, (1, 2, 3, 9)) for P in (11, 16) for n in (17, 257, 1597)])


@pytest.mark.parametrize("kernel,P,n,sizes", C_EXACT, ids=["%s-P%d-n%d" % c[:3] for c in C_EXACT])
def test_subfin_avg_exact_sums_bitwise(kernel, P, n, sizes):
    """theta = K Sop^T with exact-sum inputs -- Sop: integers in [-8, 8] times 2^-8, K: integers in [-7, 7]; n <= 1597 terms of at most
    56 x 2^-8, exact in any order -- equal to NumPy's product at every element, S * P written and nothing behind it.
    subfin_avg_small_kernel (n <= 16: a thread per sample; S around one workgroup of 256), subfin_avg_kernel<10, 4> (P <= 10: four
    samples per wave, four waves per workgroup -- S = 1..5, 17 are the tails of both; n = 17 the dispatch boundary, n % 256 the tail of
    the four 64-column passes) and subfin_avg_kernel<16, 2> (10 < P <= 16: two samples per wave)."""
    from bayesianinferencedl_amd.engine import SubfinAverager
    assert {"small": n <= 16, "10x4": n > 16 and P <= 10, "16x2": n > 16 and 10 < P <= 16}[kernel]
    rng = np.random.default_rng(100 * P + n)
    Si, Ki = rng.integers(-8, 9, (P, n)), rng.integers(-7, 8, (max(sizes), n))
    Sop, K = Si * GRID, Ki.astype(np.float64)
    ref = K @ Sop.T
    assert np.array_equal(ref, (Ki @ Si.T).astype(np.float64) * GRID), "the exact-sum inputs are not exact"
    avg = SubfinAverager(Sop)
    for S in sizes:
        got = avg(K[:S])
        assert got.shape == (S, P) and np.array_equal(got, ref[:S]), (kernel, P, n, S, np.argwhere(got != ref[:S])[:4])
        assert np.array_equal(_avg_padded(avg, K[:S]), ref[:S]), (kernel, P, n, S)


@pytest.mark.parametrize("P,n", [(9, 1597), (16, 1597), (9, 4101)])
def test_subfin_avg_real_inputs_within_the_dot_product_bound_of_longdouble(P, n):
    """Sop standard normal, K = exp(0.3 N(0, 1)) [17, n] against the product in np.longdouble: per element
        |theta - theta_ref| <= n u (|Sop| @ |K|^T),   u = 2^-53,
    the first-order worst case of an n-term dot product in any order (one dropped term is about 1 / n of the sum of magnitudes, 1e9
    times the bound).  Largest ratio to the bound measured on an MI355X, (P, n) = (9, 1597) / (16, 1597) / (9, 4101): 1.25e-4 / 1.28e-4
    / 3.68e-5; NumPy's own fp64 product with these inputs: 2.5e-4 / 3.4e-4 / 8.3e-5."""
    from bayesianinferencedl_amd.engine import SubfinAverager
    rng = np.random.default_rng(P * n)
    Sop, K = rng.standard_normal((P, n)), np.exp(0.3 * rng.standard_normal((17, n)))
    ref = K.astype(np.longdouble) @ Sop.T.astype(np.longdouble)
    bound = n * U53 * (np.abs(K) @ np.abs(Sop).T)
    got = SubfinAverager(Sop)(K)
    ratio = float(np.max((np.abs(got - ref) / bound).astype(np.float64)))
    print("subfin_avg P = %d n = %d: largest |theta - theta_ref| / bound = %.2e" % (P, n, ratio))
    assert ratio <= 1.0, (P, n, ratio)


@pytest.mark.parametrize("P,n", [(9, 16), (9, 1597), (16, 1597)], ids=["small", "10x4", "16x2"])
def test_subfin_avg_rows_do_not_depend_on_their_neighbours(P, n):
    """Real inputs, S = 17, each of the three kernels: row s of the batch is bitwise the row computed alone, and a NaN sample (5: inside
    a wave's group of four and of two samples; 16: the last, alone in its wave) comes back NaN and leaves every other sample
    bit-identical."""
    from bayesianinferencedl_amd.engine import SubfinAverager
    rng = np.random.default_rng(P + n)
    Sop, K = rng.standard_normal((P, n)), np.exp(0.3 * rng.standard_normal((17, n)))
    avg = SubfinAverager(Sop)
    batch = avg(K).copy()
    assert not np.isnan(batch).any()
    for s in range(17):
        assert np.array_equal(avg(K[s:s + 1])[0], batch[s]), (P, n, s)
    bad = np.array([5, 16])
    good = np.setdiff1d(np.arange(17), bad)
    Kn = K.copy()
    Kn[bad] = NAN
    dirty = avg(Kn)
    assert np.isnan(dirty[bad]).all() and np.array_equal(dirty[good], batch[good]), (P, n)


def test_subfin_avg_refuses_more_than_sixteen_averages():
    from bayesianinferencedl_amd._ffi import FinromError
    from bayesianinferencedl_amd.engine import SubfinAverager
    for n in (5, 40):
        with pytest.raises(FinromError, match="subfin_avg: P > 16"):
            SubfinAverager(np.ones((17, n)))(np.ones((3, n)))


# ---- D. Philox normals and the seeded draw ---------------------------------------------------------------------------------------
def _diagonal(n):
    return np.diag(np.linspace(0.5, 2.0, n))


def _assert_draw(smp, d, seed, first, S):
    k, xi = smp.draw(seed, first, S, want_xi=True)
    ref = O.philox_normal(seed, first, S, smp.n)
    err = float(np.max(np.abs(xi - ref)))
    print("philox n = %d seed = %d first = %d S = %d: max |xi - oracle| = %.3g" % (smp.n, seed, first, S, err))
    assert err <= 1e-13, (smp.n, seed, first, S, err)
    assert np.max(np.abs(k / np.exp(0.5 * ref * d) - 1.0)) <= 1e-13           # (diagonal U: one product per field)


@pytest.mark.parametrize("first", [0, (1 << 32) - 2, (1 << 40) + 3])
@pytest.mark.parametrize("n", [1, 2, 5, 245])
def test_philox_normals_match_the_oracle(n, first):
    """FieldSampler.draw(want_xi=True) under a diagonal U: xi within 1e-13 absolute of oracle.fin_oracle.philox_normal (the bound of
    tests/test_gpu_parity.py and tests/test_gpu_hmc_rng.py).  n = 1 (one pair, its second half not written), 2, 5 (odd), 245; S = 4
    from first = 0, 2^32 - 2 (the sample index crosses 32 bits inside the batch) and 2^40 + 3; seeds below and above 2^32 and 2^63."""
    from bayesianinferencedl_amd.engine import FieldSampler
    d = np.linspace(0.5, 2.0, n)
    smp = FieldSampler(_diagonal(n))
    for seed in SEEDS:
        _assert_draw(smp, d, seed, first, 4)


def test_philox_normals_under_the_capped_grid():
    """n = 4101, S = 2046: 2046 x 2051 = 4 196 346 pairs, more than the GRID_CAP x 256 = 4 194 304 threads of launch_philox_normal's
    capped grid, so the grid-stride loop takes a second trip; the same bound."""
    from bayesianinferencedl_amd.engine import FieldSampler
    n, S = 4101, 2046
    assert S * ((n + 1) // 2) > GRID_CAP * 256
    _assert_draw(FieldSampler(_diagonal(n)), np.linspace(0.5, 2.0, n), SEEDS[2], (1 << 32) - 1000, S)


def test_seeded_draw_does_not_depend_on_its_cut_into_pieces():
    """finrom_sampler_draw_seeded without xi back cuts the batch into pieces of 32768 samples: S = 32768 + 3 at n = 2 takes two, the
    same draw with want_xi=True one -- bitwise equal fields; and a draw from first + 32768 continues at row 32768."""
    from bayesianinferencedl_amd.engine import FieldSampler
    n, S, seed, first = 2, 32768 + 3, SEEDS[3], (1 << 32) - 5
    smp = FieldSampler(_diagonal(n))
    pieces = smp.draw(seed, first, S)
    whole, xi = smp.draw(seed, first, S, want_xi=True)
    assert pieces.shape == (S, n) and np.array_equal(pieces, whole)
    assert np.max(np.abs(xi[32760:] - O.philox_normal(seed, first + 32760, S - 32760, n))) <= 1e-13
    tail = smp.draw(seed, first + 32768, 4)
    assert np.array_equal(tail[:3], pieces[32768:])
    assert not np.array_equal(tail[:3], pieces[:3])


# ---- E. difference kernel --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("count", [0, 1, 255, 256, 257, 2048 * 256 + 1])
def test_device_sub_is_the_difference_bitwise(count):
    """finrom_sub through engine.device_sub: bitwise a - b; 2048 x 256 + 1 elements: one more than the capped grid's threads, so the
    grid-stride loop takes a second trip.  Through ctypes into a NaN-filled buffer: nothing written behind `count`."""
    import torch
    from bayesianinferencedl_amd import _ffi
    from bayesianinferencedl_amd.engine import device_sub
    rng = np.random.default_rng(count)
    a, b = rng.standard_normal(count), rng.standard_normal(count) * 10.0 ** rng.integers(-3, 4, count)
    at, bt = _cuda(a), _cuda(b)
    got = device_sub(at, bt)
    assert got.shape == at.shape and np.array_equal(got.cpu().numpy(), a - b)
    out = torch.full((count + PAD,), NAN, dtype=torch.float64, device=at.device)
    _ffi.check(_ffi.lib().finrom_sub(at.data_ptr(), bt.data_ptr(), count, out.data_ptr(), _stream()), "finrom_sub")
    out = out.cpu().numpy()
    assert np.isnan(out[count:]).all(), "finrom_sub wrote behind count"
    assert np.array_equal(out[:count], a - b)
