"""The counter-based random stream of the HMC chains (hmc.py rng="philox"), in NumPy: what finrom_hmc_draw (csrc/util_kernels.hip::
hmc_draw_kernel) draws on the device, restated for the host recursion `hmc.run_chains`.

For the chain with seed s (0 <= s < 2^64) and GLOBAL proposal index p, Philox4x32-10 (Salmon et al., SC'11) with key (s lo, s hi):
  * momentum: counter (p lo, p hi, pair index jb, 0); the output words (o1 o0) and (o3 o2) give two 53-bit uniforms u1 in (0, 1] and
    u2 in [0, 1), and Box-Muller turns them into the standard normals xi[2 jb], xi[2 jb + 1] (for odd n the last pair gives one);
  * Metropolis uniform: counter (p lo, p hi, 0, 1); a = (o1 << 32) | o0, u = ((a >> 11) + 1) 2^-53 in (0, 1], lu = log u <= 0, finite;
  * second-stage uniform (hmc.py correct=, finrom_hmc_draw_stage2): counter (p lo, p hi, 0, 2), the same conversion.
  * the No-U-turn transition (hmc.py nuts=, nuts.py; on the device drawn inside finrom_hmc_nuts_ml): doubling j: counter (p lo, p hi, j,
    3), direction = o2 & 1 (1: forward), u_top from (o1 o0); leaf m = 1, 2, ...: counter (p lo, p hi, m, 4), u_m from (o1 o0); both
    uniforms (a >> 11) 2^-53 in [0, 1);
A draw depends on (s, p) and on nothing else: a chain is the same for any block size, any deal of the chains over ranks, and for a
run continued from its end state at the proposal index it stopped at."""
from __future__ import annotations

import numpy as np

_M32 = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)
_TWO_PI = 6.283185307179586476925286766559


def philox4x32_10(c, k0, k1):
    """Ten rounds of Philox4x32.  c: four uint64 arrays (or scalars) holding 32-bit counter words; k0, k1: the key words, scalars or
    arrays that broadcast against them.  Returns the four output words as uint64 arrays."""
    c = [np.asarray(w, dtype=np.uint64) for w in c]
    k0, k1 = np.asarray(k0, dtype=np.uint64), np.asarray(k1, dtype=np.uint64)
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c[0]
        p1 = np.uint64(0xCD9E8D57) * c[2]
        c = [(p1 >> _S32) ^ c[1] ^ k0, p1 & _M32, (p0 >> _S32) ^ c[3] ^ k1, p0 & _M32]
        k0 = (k0 + np.uint64(0x9E3779B9)) & _M32
        k1 = (k1 + np.uint64(0xBB67AE85)) & _M32
    return c


def check_seeds(seeds):
    """The seeds as a uint64 array [C]; ValueError for one outside [0, 2^64)."""
    out = np.empty(len(seeds), dtype=np.uint64)
    for i, s in enumerate(seeds):
        s = int(s)
        if not 0 <= s < 1 << 64:
            raise ValueError(f"rng='philox': seed {s} is outside [0, 2^64)")
        out[i] = s
    return out


def _words(seeds, first, B):
    """Key words [1, C, 1] and proposal-index words [B, 1, 1] of a block."""
    s = check_seeds(seeds)[None, :, None]
    first = int(first)
    if first < 0 or first + B > 1 << 63:
        raise ValueError(f"rng='philox': proposals {first} .. {first + B} are outside [0, 2^63)")
    p = (np.uint64(first) + np.arange(B, dtype=np.uint64))[:, None, None]
    return s & _M32, s >> _S32, p & _M32, p >> _S32


def draw_block(seeds, first, B, n):
    """The draws of proposals first .. first + B - 1 for the chains with `seeds` [C]: (P [B, C, n] standard normals, lu [B, C]
    log-uniforms), row [j, c] being proposal first + j of chain c -- the block finrom_hmc_draw writes."""
    n, B = int(n), int(B)
    if n < 1 or B < 0:
        raise ValueError("draw_block: n < 1 or B < 0")
    k0, k1, p_lo, p_hi = _words(seeds, first, B)
    C = k0.shape[1]
    npair = (n + 1) // 2
    shape = (B, C, npair)
    jb = np.arange(npair, dtype=np.uint64)[None, None, :]
    o = philox4x32_10([np.broadcast_to(p_lo, shape), np.broadcast_to(p_hi, shape), np.broadcast_to(jb, shape),
                       np.zeros(shape, np.uint64)], k0, k1)
    a = (o[1] << _S32) | o[0]
    b = (o[3] << _S32) | o[2]
    u1 = ((a >> np.uint64(11)) + np.uint64(1)).astype(np.float64) * 2.0 ** -53          # (0, 1]
    u2 = (b >> np.uint64(11)).astype(np.float64) * 2.0 ** -53                            # [0, 1)
    rad = np.sqrt(-2.0 * np.log(u1))
    ang = _TWO_PI * u2
    P = np.empty((B, C, 2 * npair))
    P[..., 0::2] = rad * np.cos(ang)
    P[..., 1::2] = rad * np.sin(ang)
    shape = (B, C, 1)
    o = philox4x32_10([np.broadcast_to(p_lo, shape), np.broadcast_to(p_hi, shape), np.zeros(shape, np.uint64),
                       np.ones(shape, np.uint64)], k0, k1)
    a = ((o[1] << _S32) | o[0])[..., 0]
    lu = np.log(((a >> np.uint64(11)) + np.uint64(1)).astype(np.float64) * 2.0 ** -53)
    return np.ascontiguousarray(P[..., :n]), lu


def draw_block_stage2(seeds, first, B):
    """The SECOND log-uniforms of proposals first .. first + B - 1 for the chains with `seeds` [C]: lu2 [B, C], what
    finrom_hmc_draw_stage2 writes (hmc.py correct=: the second stage's test).  Counter (p lo, p hi, 0, 2), the conversion of
    draw_block's log-uniform: finite and <= 0, a function of (seed, p) alone."""
    B = int(B)
    if B < 0:
        raise ValueError("draw_block_stage2: B < 0")
    k0, k1, p_lo, p_hi = _words(seeds, first, B)
    shape = (B, k0.shape[1], 1)
    o = philox4x32_10([np.broadcast_to(p_lo, shape), np.broadcast_to(p_hi, shape), np.zeros(shape, np.uint64),
                       np.full(shape, 2, np.uint64)], k0, k1)
    a = ((o[1] << _S32) | o[0])[..., 0]
    return np.log(((a >> np.uint64(11)) + np.uint64(1)).astype(np.float64) * 2.0 ** -53)


def momentum(seed, p, n):
    """The standard normals xi [n] of proposal p of the chain with `seed`."""
    return draw_block([seed], p, 1, n)[0][0, 0]


def log_uniform(seed, p):
    """log u of the Metropolis test of proposal p of the chain with `seed`: finite and <= 0."""
    return float(draw_block([seed], p, 1, 1)[1][0, 0])


def _nuts_words(seed, p, index, word):
    """The output words of counter (p lo, p hi, index, word) under the key `seed`, as Python ints."""
    s = int(check_seeds([seed])[0])
    p, index = int(p), int(index)
    if not 0 <= p < 1 << 63 or not 0 <= index < 1 << 32:
        raise ValueError(f"rng='philox': proposal {p} or index {index} is out of range")
    o = philox4x32_10([p & 0xFFFFFFFF, p >> 32, index, word], s & 0xFFFFFFFF, s >> 32)
    return [int(w) for w in o]


def nuts_top(seed, p, j):
    """Doubling j of the NUTS transition (nuts.py) of proposal p of the chain with `seed`: counter (p lo, p hi, j, 3) ->
    (forward: o2 & 1, u_top = ((o1 o0) >> 11) 2^-53 in [0, 1)).  A function of (seed, p, j) alone."""
    o = _nuts_words(seed, p, j, 3)
    return bool(o[2] & 1), float(((o[1] << 32) | o[0]) >> 11) * 2.0 ** -53


def nuts_leaf(seed, p, m):
    """Leaf m = 1, 2, ... of that transition: counter (p lo, p hi, m, 4) -> u_m = ((o1 o0) >> 11) 2^-53 in [0, 1)."""
    o = _nuts_words(seed, p, m, 4)
    return float(((o[1] << 32) | o[0]) >> 11) * 2.0 ** -53
