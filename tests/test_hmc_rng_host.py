"""The counter-based random stream of the HMC chains (hmc.py rng="philox") on the host: philox.py against the oracle's NumPy
restatement of the device draw bit for bit, the Metropolis uniform's definition, block-cut / chain-deal / continuation invariance of
`hmc.run_chains` on a closed-form potential, the refusals, and finrom_hmc_draw's argument checks -- no GPU needed."""
import ctypes as C

import numpy as np
import pytest

from oracle import fin_oracle as O

BIG_SEED = (1 << 32) + 7
FIRSTS = (0, (1 << 32) - 2, (1 << 33) + 7)


@pytest.mark.parametrize("n", [1, 2, 5, 1597])
@pytest.mark.parametrize("first", FIRSTS)
def test_momentum_and_draw_block_are_the_oracles_philox_normal(n, first):
    """philox.momentum(seed, p, n) == O.philox_normal(seed, p, 1, n)[0] and draw_block's rows == O.philox_normal(seed, first, B, n),
    bit for bit; seeds include one above 2^32 and one with the top bit set; `first` crosses 2^32."""
    from bayesianinferencedl_amd.bayesian_inference import philox
    seeds = [0, 7, BIG_SEED, (1 << 63) + 1]
    B = 3
    P, lu = philox.draw_block(seeds, first, B, n)
    assert P.shape == (B, len(seeds), n) and lu.shape == (B, len(seeds)) and P.dtype == lu.dtype == np.float64
    for c, s in enumerate(seeds):
        assert np.array_equal(P[:, c], O.philox_normal(s, first, B, n)), (s, first, n)
        for j in range(B):
            assert np.array_equal(philox.momentum(s, first + j, n), O.philox_normal(s, first + j, 1, n)[0]), (s, first, j, n)
            assert philox.log_uniform(s, first + j) == lu[j, c]


def test_philox4x32_10_is_the_oracles():
    from bayesianinferencedl_amd.bayesian_inference import philox
    rng = np.random.default_rng(0)
    c = [rng.integers(0, 1 << 32, 50, dtype=np.uint64) for _ in range(4)]
    got, want = philox.philox4x32_10(c, 0xA4093822, 0x299F31D0), O.philox4x32_10(c, 0xA4093822, 0x299F31D0)
    assert all(np.array_equal(g, w) for g, w in zip(got, want))


def test_log_uniform_is_its_definition_finite_and_nonpositive():
    """lu = log(((a >> 11) + 1) 2^-53), a = (o1 << 32) | o0 of Philox4x32-10 at counter (p lo, p hi, 0, 1), key (seed lo, hi); over
    10^5 draws (100 proposals from each `first`, 334 chains) it is finite and <= 0."""
    from bayesianinferencedl_amd.bayesian_inference import philox
    for s in (0, 7, BIG_SEED, (1 << 64) - 1):
        for p in (0, 5, (1 << 32) - 1, (1 << 33) + 7):
            o = O.philox4x32_10([np.uint64(p & 0xFFFFFFFF), np.uint64(p >> 32), np.uint64(0), np.uint64(1)], s & 0xFFFFFFFF, s >> 32)
            a = (int(o[1]) << 32) | int(o[0])
            assert philox.log_uniform(s, p) == np.log(np.float64((a >> 11) + 1) * 2.0 ** -53), (s, p)
    seeds = [BIG_SEED * c + c for c in range(334)]
    total = 0
    for first in FIRSTS:
        lu = philox.draw_block(seeds, first, 100, 1)[1]
        assert np.all(np.isfinite(lu)) and np.all(lu <= 0.0)
        total += lu.size
    assert total >= 10 ** 5


def test_seeds_that_differ_in_the_high_word_give_different_rows():
    from bayesianinferencedl_amd.bayesian_inference import philox
    P, lu = philox.draw_block([5, 5 + (1 << 32), 5 + (1 << 63)], 3, 2, 64)
    for a, b in ((0, 1), (0, 2), (1, 2)):
        assert not np.any(P[:, a] == P[:, b]) and not np.any(lu[:, a] == lu[:, b])


def test_draw_block_does_not_depend_on_the_cut_or_the_deal():
    from bayesianinferencedl_amd.bayesian_inference import philox
    seeds = [0, 7, BIG_SEED, (1 << 63) + 1]
    P, lu = philox.draw_block(seeds, 7, 5, 11)
    Pa, la = philox.draw_block(seeds, 7, 2, 11)
    Pb, lb = philox.draw_block(seeds, 9, 3, 11)
    assert np.array_equal(P, np.concatenate([Pa, Pb])) and np.array_equal(lu, np.concatenate([la, lb]))
    Ps, ls = philox.draw_block([seeds[1], seeds[3]], 7, 5, 11)
    assert np.array_equal(Ps, P[:, [1, 3]]) and np.array_equal(ls, lu[:, [1, 3]])


def _quadratic(n):
    """A closed-form value_and_grad: loss = sum_i a_i (k_i - b_i)^2 / 2, row-wise."""
    a = np.linspace(0.5, 2.0, n)
    b = np.cos(np.arange(n))

    def f(K):
        d = K - b
        return 0.5 * np.einsum("cn,n,cn->c", d, a, d), a * d, np.zeros(len(K), bool)
    return f


N, KW = 9, dict(eps=0.35, n_leapfrog=4, sigma=1.0, tau=2.0, keep_trace=True)


def _k0(C=4):
    return np.random.default_rng(3).standard_normal((C, N))


def test_host_chains_continue_bit_for_bit():
    """6 proposals == 3 proposals, then 3 more from the end state K with proposal0=3 and the first run's mean."""
    from bayesianinferencedl_amd.bayesian_inference import hmc
    f, K0, seeds = _quadratic(N), _k0(), [100, 101, BIG_SEED, (1 << 63) + 1]
    whole = hmc.run_chains(f, K0, 1 + 6 * 4, seeds=seeds, rng="philox", mean=K0, **KW)
    assert whole.proposals == 6 and 0 < whole.accept.sum() < 4 * 6, whole.accept          # (both branches of the Metropolis test run)
    one = hmc.run_chains(f, K0, 1 + 3 * 4, seeds=seeds, rng="philox", mean=K0, **KW)
    two = hmc.run_chains(f, one.K, 1 + 3 * 4, seeds=seeds, rng="philox", mean=K0, proposal0=3, **KW)
    assert one.proposals == two.proposals == 3
    assert np.array_equal(two.K, whole.K) and np.array_equal(one.accept + two.accept, whole.accept)
    assert np.array_equal(one.trace, whole.trace[:4]) and np.array_equal(two.trace, whole.trace[3:])
    # without proposal0 the second run draws proposals 0..2 again: another chain
    again = hmc.run_chains(f, one.K, 1 + 3 * 4, seeds=seeds, rng="philox", mean=K0, **KW)
    assert not np.array_equal(again.K, whole.K)


def test_host_chains_do_not_depend_on_the_deal():
    """Chains [1, 3] run alone are rows 1 and 3 of chains [0..3]."""
    from bayesianinferencedl_amd.bayesian_inference import hmc
    f, K0, seeds = _quadratic(N), _k0(), [100, 101, BIG_SEED, (1 << 63) + 1]
    four = hmc.run_chains(f, K0, 25, seeds=seeds, rng="philox", **KW)
    two = hmc.run_chains(f, K0[[1, 3]], 25, seeds=[seeds[1], seeds[3]], rng="philox", **KW)
    assert np.array_equal(two.K, four.K[[1, 3]]) and np.array_equal(two.accept, four.accept[[1, 3]])
    assert np.array_equal(two.trace, four.trace[:, [1, 3]])


def test_rng_numpy_is_the_default_path():
    from bayesianinferencedl_amd.bayesian_inference import hmc
    f, K0, seeds = _quadratic(N), _k0(), [100, 101, 102, 103]
    a = hmc.run_chains(f, K0, 25, seeds=seeds, **KW)
    b = hmc.run_chains(f, K0, 25, seeds=seeds, rng="numpy", proposal0=0, **KW)
    assert np.array_equal(a.K, b.K) and np.array_equal(a.accept, b.accept) and np.array_equal(a.trace, b.trace)
    rngs = [np.random.default_rng(s) for s in seeds]                   # the stream as it always was: n normals, then one uniform
    P = np.stack([r.standard_normal(N) for r in rngs])
    c = hmc.run_chains(f, K0, 5, seeds=seeds, **dict(KW, eps=1e-9))
    assert c.proposals == 1 and np.allclose(c.trace[1], K0 + 4e-9 * P, rtol=0, atol=1e-15)
    p = hmc.run_chains(f, K0, 25, seeds=seeds, rng="philox", **KW)
    assert not np.array_equal(p.K, a.K)


@pytest.mark.parametrize("who", ["run_chains", "run_chains_device", "run_chains_fused"])
def test_refusals_come_before_any_work(who):
    """Seeds outside [0, 2^64) under "philox", proposal0 != 0 under "numpy", an unknown rng: ValueError, before the model is touched
    (the device functions get no solver at all here)."""
    from bayesianinferencedl_amd.bayesian_inference import hmc

    def touched(*a, **k):
        raise AssertionError("the model was evaluated")
    fn = getattr(hmc, who)
    first = touched if who == "run_chains" else None
    K0 = _k0(2)
    for kw in (dict(seeds=[1, -1], rng="philox"), dict(seeds=[1, 1 << 64], rng="philox"), dict(seeds=[1, 2], rng="numpy", proposal0=3),
               dict(seeds=[1, 2], proposal0=1), dict(seeds=[1, 2], rng="pcg"), dict(seeds=[1, 2], rng="philox", proposal0=-1)):
        with pytest.raises(ValueError, match="philox|rng"):
            fn(first, K0, 25, **kw)


def test_hmc_draw_validates_its_arguments_before_any_device_call():
    """finrom_hmc_draw: negative C, B or first_proposal, n < 1, a null pointer with B x C > 0 -> FINROM_ERR_ARG with a message; B == 0
    or C == 0 -> 0 without a launch (null pointers allowed).  Host-side checks, no GPU needed."""
    from bayesianinferencedl_amd import _ffi
    L = _ffi.lib()
    buf = (C.c_double * 8)()
    p = C.addressof(buf)                                               # (never dereferenced: every call below returns before a launch)
    for args, word in (((p, -1, 4, 0, 1, p, p), b"C < 0"), ((p, 1, 4, 0, -1, p, p), b"B < 0"), ((p, 1, 4, -1, 1, p, p), b"first_proposal"),
                       ((p, 1, 0, 0, 1, p, p), b"n < 1"), ((p, 1, -3, 0, 1, p, p), b"n < 1"), ((None, 1, 4, 0, 1, p, p), b"null"),
                       ((p, 1, 4, 0, 1, None, p), b"null"), ((p, 1, 4, 0, 1, p, None), b"null"),
                       ((p, 0, 0, 0, 1, p, p), b"n < 1"), ((p, 1, 4, -1, 0, p, p), b"first_proposal")):
        assert L.finrom_hmc_draw(*args, None) == -1, args
        assert word in L.finrom_last_error(), (args, L.finrom_last_error())
    assert L.finrom_hmc_draw(None, 0, 4, 0, 3, None, None, None) == 0
    assert L.finrom_hmc_draw(None, 3, 4, 0, 0, None, None, None) == 0
    assert L.finrom_deferred_count() == 0
