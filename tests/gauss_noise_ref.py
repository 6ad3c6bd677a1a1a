"""Reference of the native Gaussian move's noise (GaussianMove / MHMove in Philox mode), NumPy only: nothing here comes from
emcee_amd, and no value is fitted to what the device gives.

The contract (emcee_amd/csrc/emx_kernels.hpp, gauss_disp_row / native_gauss_pair; DESIGN.md, "The Gaussian move's noise"):

* pair p (coordinates 2p, 2p + 1) of walker w at step s under the 64-bit seed k is ONE Box-Muller pair;
* it comes from half a Philox4x32-7 block: counter (w, 2 + (p >> 1), s lo, s hi), key (k lo, k hi), words (2h, 2h + 1) with
  h = p & 1: word a = v[2h] makes the radius, word b = v[2h + 1] the direction;
* u = (f32(a) + 0.5) * 2^-32 in (0, 1] from all 32 bits, rev = f32(b >> 8) * 2^-24 in [0, 1) revolutions from the HIGH 24 bits;
  both are formed in float32 (conversion, one addition, one multiplication: IEEE operations, the same in NumPy);
* n(w, 2p) = r cos(2 pi rev), n(w, 2p + 1) = r sin(2 pi rev), r = sqrt(-2 ln u).  The device evaluates these with the f32
  hardware transcendentals; here everything after the two f32 inputs is float64;
* the displacement of coordinate d is (f * scale_d) * n(w, d), in that order (moves/gaussian.py, k_gauss_disp), f the step's
  step-size factor; in the one-coordinate modes only column col[w] of walker w moves.

Which seed and step each path hands gauss_disp_row, and how a test gets them:

* EnsembleSampler / DeviceEnsemble (k_gauss_disp, k_halfstep, k_persist_gauss, k_small_run, the DeviceFused half-step): the
  context's seed (c->ph_seed) and the step counter of the step begun (cur.nat.step), which starts where set_philox put it and
  grows by one per proposal, thinned ones included.  DeviceEnsemble.get_philox() returns (seed, next step);
  EnsembleSampler._philox_seed() is the seed of a sampler, whose first run starts at step 0.
* EnsembleBatch: member b uses its own seed, philox_seed(RandomState(seeds[b])), and the batch's common step counter from 0.
* PTSampler: rung t of object g is the batch member seeded with s[g, t] = RandomState(seeds[g]).randint(0, 2^32, ntemps,
  uint64)[t], i.e. it uses philox_seed(RandomState(s[g, t])) (emx_pt_fused.hpp: seedS[t]) and the common step counter.

philox_seed_of() below restates that seed rule (the first words of the MT19937 key) without importing the package.
"""
import numpy as np

M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
MASK = np.uint64(0xFFFFFFFF)
S32 = np.uint64(32)

STREAM_BASE = 2          # blocks 0 and 1 of a walker belong to the plans (accept uniform, column, factor)
ROUNDS = 7


def philox4x32(c0, c1, c2, c3, k0, k1, rounds):
    """Philox4x32-`rounds` (Salmon et al. 2011) on arrays (counters and keys broadcast): -> four uint32 arrays.
    Products in uint64; a round is c = (hi(M1 c2) ^ c1 ^ k0, lo(M1 c2), hi(M0 c0) ^ c3 ^ k1, lo(M0 c0)), then the key is bumped."""
    c0, c1, c2, c3, k0, k1 = np.broadcast_arrays(*[np.asarray(c).astype(np.uint64) & MASK for c in (c0, c1, c2, c3, k0, k1)])
    for _ in range(rounds):
        p0, p1 = M0 * c0, M1 * c2
        c0, c1, c2, c3 = (p1 >> S32) ^ c1 ^ k0, p1 & MASK, (p0 >> S32) ^ c3 ^ k1, p0 & MASK
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return tuple(c.astype(np.uint32) for c in (c0, c1, c2, c3))


def f32_inputs(a, b, low_bits=False):
    """the kernel's two f32 inputs, exactly: u in (0, 1], rev in [0, 1)"""
    a, b = np.asarray(a, dtype=np.uint32), np.asarray(b, dtype=np.uint32)
    u = (a.astype(np.float32) + np.float32(0.5)) * np.float32(2.0 ** -32)
    bits = (b & np.uint32(0xFFFFFF)) if low_bits else (b >> np.uint32(8))
    rev = bits.astype(np.float32) * np.float32(2.0 ** -24)
    assert u.dtype == np.float32 and rev.dtype == np.float32
    return u, rev


def words_to_normals(a, b):
    """-> (n0, n1, r) in float64 from the radius word a and the direction word b"""
    u, rev = f32_inputs(a, b)
    r = np.sqrt(-2.0 * np.log(u.astype(np.float64)))
    ang = 2.0 * np.pi * rev.astype(np.float64)
    return r * np.cos(ang), r * np.sin(ang), r


def pair_words(seed, step, w, p):
    """the (a, b) words of pair p of walker w (arrays broadcast)"""
    seed, step = int(seed) & (2 ** 64 - 1), int(step) & (2 ** 64 - 1)
    p = np.asarray(p, dtype=np.int64)
    v = philox4x32(w, STREAM_BASE + (p >> 1), step & 0xFFFFFFFF, step >> 32, seed & 0xFFFFFFFF, seed >> 32, ROUNDS)
    h = (p & 1).astype(bool)
    return np.where(h, v[2], v[0]), np.where(h, v[3], v[1])


def noise(seed, step, N, D):
    """-> (n, r): the (N, D) normals of step `step` under `seed`, and the (N, D) radius each came from"""
    npair = (D + 1) // 2
    w, p = np.meshgrid(np.arange(N), np.arange(npair), indexing="ij")
    a, b = pair_words(seed, step, w, p)
    n0, n1, r = words_to_normals(a, b)
    n = np.stack([n0, n1], axis=2).reshape(N, 2 * npair)[:, :D]
    return np.ascontiguousarray(n), np.ascontiguousarray(np.repeat(r, 2, axis=1)[:, :D])


def scale_row(scale, D):
    return np.broadcast_to(np.asarray(scale, dtype=np.float64), (D,))


def displacement(seed, step, N, D, scale, f=1.0, col=None):
    """-> (disp, r): (f * scale_d) * n in float64, in that order; with `col` (N,) only that coordinate of each walker is non-zero"""
    n, r = noise(seed, step, N, D)
    d = (np.float64(f) * scale_row(scale, D)) * n
    if col is not None:
        keep = np.arange(D)[None, :] == np.asarray(col)[:, None]
        d = np.where(keep, d, 0.0)
    return d, r


# ---- the gate (the issue's section 4) ------------------------------------------------------------------------------------------
K_GATE = 4096.0          # twelve of f32's 24 bits kept: fixed in advance, not derived from a hardware figure


def unit(scale, D, r, f=1.0):
    """|f s_d| 2^-24 r: what an error is measured in"""
    return np.abs(np.float64(f) * scale_row(scale, D)) * 2.0 ** -24 * r


def ratio(d, d_ref, r, scale, f=1.0, extra=0.0):
    """(|d - d_ref| - 2^-52 |d_ref| - extra) / (|f s_d| 2^-24 r), >= 0: the gate asks for <= K.  Where the radius is 0 (u == 1)
    the reference is 0 and so must d be, up to `extra`: the ratio is then 0 or inf."""
    return ratio_units(d, d_ref, unit(scale, d_ref.shape[-1], r, f), extra)


def ratio_units(d, d_ref, den, extra=0.0):
    """ratio() with the unit given (a sum of several steps' units where the difference of two stored rows spans several steps)"""
    over = np.maximum(np.abs(d - d_ref) - 2.0 ** -52 * np.abs(d_ref) - extra, 0.0)
    den = np.broadcast_to(den, over.shape)
    out = np.zeros(over.shape)
    np.divide(over, den, out=out, where=den > 0)
    out[(den == 0) & (over > 0)] = np.inf
    return out


def philox_seed_of(seed):
    """the Philox seed of a chain seeded with the integer `seed`: the first words of RandomState(seed)'s MT19937 key"""
    key = np.random.RandomState(seed).get_state()[1]
    return (int(key[0]) << 32 | int(key[1])) ^ (int(key[2]) << 16)


# ---- mutants: float64 twins of noise() with one plausible kernel mistake each (tests/test_gauss_noise_ref_cpu.py) ---------------
def mutant_noise(kind, seed, step, N, D, G=8, scale=None):
    """(N, D) of `scale_d * n` as a kernel with the mistake `kind` would give (scale None: ones).  G: the lanes per walker of the
    row layout, which only the 'dpp_chunks' mutant depends on."""
    seed, step = int(seed) & (2 ** 64 - 1), int(step) & (2 ** 64 - 1)
    npair = (D + 1) // 2
    w, p = np.meshgrid(np.arange(N), np.arange(npair), indexing="ij")
    sl, sh, k0, k1 = step & 0xFFFFFFFF, step >> 32, seed & 0xFFFFFFFF, seed >> 32
    c0, c1, h, rounds, src = w, STREAM_BASE + (p >> 1), p & 1, ROUNDS, p
    if kind == "dpp_chunks":
        # pair c G + gl of an odd lane gl takes what belongs to the other chunk of its pair of chunks
        c, gl = p // G, p % G
        src = np.where(gl & 1 == 1, (c ^ 1) * G + gl, p)
        c1, h = STREAM_BASE + (src >> 1), src & 1
    elif kind == "halves":
        h = 1 - (p & 1)
    elif kind == "block_p":
        c1 = STREAM_BASE + p
    elif kind == "base0":
        c1 = p >> 1
    elif kind == "step_swapped":
        sl, sh = sh, sl
    elif kind == "rounds10":
        rounds = 10
    elif kind == "walker_block":
        c0, c1 = c1, c0
    v = philox4x32(c0, c1, sl, sh, k0, k1, rounds)
    a, b = np.where(h.astype(bool), v[2], v[0]), np.where(h.astype(bool), v[3], v[1])
    u, rev = f32_inputs(a, b, low_bits=(kind == "rev_low"))
    r = np.sqrt(-2.0 * np.log(u.astype(np.float64)))
    ang = 2.0 * np.pi * rev.astype(np.float64)
    n0, n1 = r * np.cos(ang), r * np.sin(ang)
    if kind == "sincos":
        n0, n1 = n1, n0
    n = np.stack([n0, n1], axis=2).reshape(N, 2 * npair)[:, :D]
    s = np.ones(D) if scale is None else scale_row(scale, D)
    if kind == "scale_next":
        s = np.concatenate([s[1:], s[:1]])
    return s * n


MUTANTS = ("halves", "block_p", "base0", "step_swapped", "rounds10", "walker_block", "sincos", "rev_low", "scale_next", "dpp_chunks")
