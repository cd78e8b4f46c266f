"""Argument sets of the per-function probes (fyprt_selftest_functions on the device, orc_probe in the oracle): for every probe one
seeded bulk array and an explicit edge list, as rows of 32-bit words in the layouts of include/fyprt.h.  Shared by
tests/test_gpu_functions.py (device against oracle, bit for bit) and tests/test_functions_cpu.py (the non-vacuity conditions on the
oracle's outputs, which need no GPU)."""
import itertools

import numpy as np

from fypraytracer_amd import capi

F, U = np.float32, np.uint32
BULK = 1 << 20                      # records of a bulk array (the issue's upper limit)
KPI = F(3.1415926535)               # rt_math.h / MathUtils.cuh:17
NAN, INF = F(np.nan), F(np.inf)
DENORM_MIN, DENORM_MAX = np.array([1, 0x007FFFFF], dtype=U).view(F)


def bits(a):
    return np.ascontiguousarray(a, dtype=F).view(U)


def from_bits(b):
    return np.ascontiguousarray(b, dtype=U).view(F)


def around(x, ulps=1):
    """x and its neighbours up to `ulps` away on either side (bit pattern steps; x finite and not zero)"""
    b = int(bits([x])[0])
    return from_bits(np.arange(b - ulps, b + ulps + 1, dtype=np.int64).astype(U))


def rows(*cols):
    """(count, words) uint32 array from columns / column blocks of float32 or uint32"""
    parts = []
    for c in cols:
        c = np.asarray(c)
        c = c.reshape(len(c), -1)
        parts.append(c.view(U) if c.dtype == F else c.astype(U))
    return np.ascontiguousarray(np.concatenate(parts, axis=1))


# ---------------------------------------------------------------------------------------------- pcg_hash and its inverse
def pcg_hash(x):
    state = (int(x) * 747796405 + 2891336453) & 0xFFFFFFFF
    word = (((state >> ((state >> 28) + 4)) ^ state) * 277803737) & 0xFFFFFFFF
    return (word >> 22) ^ word


def pcg_unhash(y):
    """the seed whose pcg_hash is y (the hash is a bijection: an LCG step, an xorshift by 4 + the top nibble, an odd multiply, an xorshift by 22)"""
    word = int(y) ^ (int(y) >> 22)
    t = (word * pow(277803737, -1, 1 << 32)) & 0xFFFFFFFF
    s = (t >> 28) + 4                                           # the top nibble passes through the xorshift unchanged
    state = t
    for _ in range(8):
        state = t ^ (state >> s)
    return ((state - 2891336453) * pow(747796405, -1, 1 << 32)) & 0xFFFFFFFF


# rnd() = float(hash) * 2^-32: hash 0 gives exactly 0; 0xFFFFFF80 is the smallest hash that rounds up to 2^32, i.e. to u == 1.0
SEED_U_ZERO, SEED_U_BELOW_ONE, SEED_U_ONE, SEED_U_ONE_MAX = (pcg_unhash(h) for h in (0, 0xFFFFFF7F, 0xFFFFFF80, 0xFFFFFFFF))
SEED_U2_ZERO, SEED_U2_ONE = pcg_unhash(SEED_U_ZERO), pcg_unhash(SEED_U_ONE)            # the SECOND draw is 0 / 1.0


# ---------------------------------------------------------------------------------------------- scalar probes
def sincos_inputs(rng):
    """The domain is what the renderer can reach — sincos_f's header: "valid for xf in [0, 2*pi + eps] (2*pi*u) and small positive
    angles": x = 2.0f * kPi * u with u = float(seed) * 2^-32 in [0, 1].  No negative and no huge angles are fed (not valid there)."""
    two_pi = F(2.0) * KPI
    u = rng.integers(0, 1 << 32, BULK, dtype=np.uint64).astype(F) * F(2.0 ** -32)
    bulk = two_pi * u
    ue = np.array([0.0, 2.0 ** -32, 1.0, np.nextafter(F(1), F(0))], dtype=F)
    edge = [two_pi * ue]
    for k in range(5):                                          # every float within 256 ulp of k*pi/2: rint() changes quadrant there
        c = F(k * (np.pi / 2))
        edge.append(from_bits(np.arange(0, 257, dtype=U)) if k == 0 else around(c, 256))      # k = 0: the non-negative side only
    return rows(bulk), rows(np.concatenate(edge))


def acos_inputs(rng):
    bulk = rng.uniform(-1.0, 1.0, BULK).astype(F)
    e = [[0.0, -0.0, 2.0, -2.0, INF, -INF, NAN, DENORM_MIN, -DENORM_MIN, DENORM_MAX, -DENORM_MAX]]
    for c in (0.5, -0.5, 1.0, -1.0):                            # both neighbours of +-1: one of each pair is just outside -> NaN
        e.append(around(F(c)))
    return rows(bulk), rows(np.concatenate([np.asarray(x, dtype=F) for x in e]))


def pow5_inputs(rng):
    bulk = rng.uniform(0.0, 1.0, BULK).astype(F)
    # x^5 is denormal in binary32 for 2^-29.8 <= x < 2^-25.2, and rounds to 0 / the smallest denormal around 2^-30
    e = np.array([0.0, DENORM_MIN, DENORM_MAX, 1.0, np.nextafter(F(1), F(0)), 2.0 ** -25, 2.0 ** -26, 1e-8, 3e-9, 2.0 ** -29, 1.1e-9,
                  2.0 ** -29.8, 2.0 ** -30, 2.0 ** -31, 1.5 * 2.0 ** -26, 2.0 ** -25.2], dtype=F)
    return rows(bulk), rows(e)


def rnd_inputs(rng):
    bulk = rng.integers(0, 1 << 32, BULK, dtype=np.uint64).astype(U)
    e = np.array([0, 1, 0xFFFFFFFF, 0xFFFFFF7F, 0xFFFFFF80, SEED_U_ZERO, SEED_U_BELOW_ONE, SEED_U_ONE, SEED_U_ONE_MAX], dtype=U)
    return rows(bulk), rows(e)


def unit_vectors(rng, n):
    v = rng.normal(size=(n, 3))
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(F)


def oct_encode_inputs(rng):
    bulk = unit_vectors(rng, BULK)
    e = []
    for pos in range(3):                                        # (+-0, +-0, +-1) and its permutations: the six axes with every sign of zero
        for sx, sy, sz in itertools.product((1.0, -1.0), repeat=3):
            v = [sx * 0.0, sy * 0.0]
            v.insert(pos, sz * 1.0)
            e.append(v)
    for t in np.linspace(0.0, 2 * np.pi, 17):                   # the z = 0 seam, from either side of zero
        for z in (0.0, -0.0, float(DENORM_MIN), -float(DENORM_MIN), -1e-8):
            e.append([np.cos(t), np.sin(t), z])
    e += [[0.0, 0.0, 0.0], [-0.0, -0.0, -0.0], [0.5, -0.0, -0.5], [-0.0, 0.5, -0.5], [0.0, 0.5, -0.5], [-0.3, -0.0, -0.7]]      # zero vector -> NaN
    return rows(bulk), rows(np.array(e, dtype=F))


def oct_decode_inputs(rng):
    bulk = rng.uniform(-1.0, 1.0, (BULK, 2)).astype(F)
    e = [[0.5, 0.5], [0.25, -0.75], [-0.75, 0.25], [-0.5, -0.5], [1.0, 0.0], [0.0, 1.0], [-1.0, -0.0], [-0.0, -1.0], [1.0, -0.0], [-0.0, 1.0],
         [0.0, 0.0], [-0.0, 0.0], [0.0, -0.0], [-0.0, -0.0], [-0.0, 0.3], [0.3, -0.0], [0.8, 0.8], [-0.8, 0.8], [-0.0, 1.0000001], [1.0000001, -0.0],
         [0.0, 1.0000001], [1.0, 1.0], [-1.0, -1.0], [1.0, -1.0], [0.5, 0.50000006], [-0.0, -1.5]]         # |x| + |y| = 1, -0.0 through the sign tests
    return rows(bulk), rows(np.array(e, dtype=F))


def pack_inputs(rng):
    bulk = rng.uniform(-0.5, 1.5, (BULK, 4)).astype(F)
    v = [np.array([0.0, -0.0, -1.0, -1e-8, -float(DENORM_MIN), 1.0, 1.5, 2.0, 1e30, INF, -INF, NAN, 0.5], dtype=F)]
    for k in (0, 1, 127, 128, 254, 255):
        c = F(k) / F(255)
        v.append(from_bits([0x80000001, 0, 1]) if k == 0 else around(c))
    v = np.concatenate(v)
    edge = np.stack([np.roll(v, -j) for j in range(4)], axis=1)       # every edge value in every channel
    return rows(bulk), rows(edge)


def unpack_inputs(rng):
    bulk = rng.integers(0, 1 << 32, BULK, dtype=np.uint64).astype(U)
    b = np.arange(256, dtype=U)
    e = np.concatenate([b * U(0x01010101), b, b << U(8), b << U(16), b << U(24)])                # all 256 byte values, in every channel
    return rows(bulk), rows(e)


def asin_kernel_inputs(rng):
    """binary64 in, binary64 out (low word first): acos_f passes z = x * x for |x| <= 0.5 and (1 - |x|) / 2 beyond, both in [0, 0.25]"""
    bulk = rng.uniform(0.0, 0.25, BULK)
    e = np.array([0.0, -0.0, 0.25, np.nextafter(0.25, 0.0), 5e-324, 2.0 ** -1022, 2.0 ** -60, 2.0 ** -30, 1e-300, 0.125, 0.0625, 1.0 / 3.0 * 0.25])
    return np.ascontiguousarray(bulk.view(U).reshape(-1, 2)), np.ascontiguousarray(e.view(U).reshape(-1, 2))


# ---------------------------------------------------------------------------------------------- surface records (BRDF, pdfs, samplers)
def surface_bulk(rng, n=BULK):
    N = unit_vectors(rng, n)

    def upper(v):
        d = np.sum(v.astype(np.float64) * N, axis=1, keepdims=True)
        return np.where(d < 0, -v, v).astype(F)
    V, L = upper(unit_vectors(rng, n)), upper(unit_vectors(rng, n))
    albedo = rng.uniform(0.0, 1.0, (n, 3)).astype(F)
    pick = rng.integers(0, 3, n)
    metallic = np.where(pick == 0, 0.0, np.where(pick == 1, 1.0, rng.uniform(0.0, 1.0, n))).astype(F)
    roughness = rng.uniform(0.0, 1.0, n).astype(F)
    seed = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(U)
    return rows(N, V, L, albedo, metallic, roughness, seed, np.zeros(n, dtype=U))


def _nrm(v):
    v = np.asarray(v, dtype=np.float64)
    return (v / np.linalg.norm(v)).astype(F)


def surface_geometries():
    """(N, V, L) triples of the edge list"""
    g = []
    s = F(np.sqrt(0.5))
    for N in (_nrm([0.3, 0.8, -0.52]), np.array([0, 1, 0], dtype=F), np.array([0, 0, 1], dtype=F), np.array([1, 0, 0], dtype=F),
              np.array([0, -1, 0], dtype=F), np.array([s, 0, s], dtype=F), np.array([-s, 0, s], dtype=F)):   # the last four rows: n.x^2 == n.z^2, the tie in onb()
        # two directions in the upper hemisphere of N, one exactly perpendicular to it
        a = np.cross(N.astype(np.float64), [0.9, 0.1, 0.42]); a = _nrm(a)
        up1, up2 = _nrm(N + 0.7 * a), _nrm(1.3 * N - 0.4 * a + 0.2 * np.cross(N, a))
        perp = a if abs(float(np.dot(a, N))) == 0.0 else None
        g += [(N, N, up1),                  # V = N
              (N, -up1, up2),               # V below the surface
              (N, up1, -up1),               # L = -V: H = normalize(0)
              (N, up1, up1),                # L = V
              (N, up1, up2),                # a plain case with this N (axis-aligned N: the tie in onb)
              (N, up2, N)]                  # L = N
        if perp is not None:
            g += [(N, perp, up1), (N, up1, perp), (N, perp, perp)]        # V perpendicular to N exactly; N.L = 0 exactly
    for N, P in (([0, 1, 0], [1, 0, 0]), ([0, 1, 0], [0, 0, 1]), ([0, 0, 1], [0, 1, 0]), ([1, 0, 0], [0, 0, -1])):     # exact by construction
        N, P = np.array(N, dtype=F), np.array(P, dtype=F)
        up = _nrm(N + 0.5 * P)
        g += [(N, P, up), (N, up, P), (N, P, P), (N, P, -P)]
    return g


SURFACE_ROUGHNESS = [0.0, 2.0 ** -20, 0.05, 1.0, 1.5]
SURFACE_METALLIC = [0.0, 2.0 ** -24, 0.5, 1.0 - 2.0 ** -24, 1.0]
SURFACE_ALBEDO = [(0.0, 0.0, 0.0), (1.0, 1.0, 1.0), (2.0, 0.5, 0.0)]


def surface_edges(seeds=(1,)):
    geo = surface_geometries()
    recs = []
    for (N, V, L), r, m, a in itertools.product(geo, SURFACE_ROUGHNESS, SURFACE_METALLIC, SURFACE_ALBEDO):
        recs.append(np.concatenate([N, V, L, np.array(a, dtype=F), np.array([m, r], dtype=F)]))
    base = np.array(recs, dtype=F)
    seeds = np.asarray(seeds, dtype=U)
    out = np.repeat(base, len(seeds), axis=0)
    return rows(out, np.tile(seeds, len(base)), np.zeros(len(out), dtype=U))


def sampler_seeds(rng):
    """64 seeds per edge case: the first draw 0 / the largest value below 1 / exactly 1.0, the second draw 0 / 1.0, and random ones"""
    special = [SEED_U_ZERO, SEED_U_BELOW_ONE, SEED_U_ONE, SEED_U2_ZERO, SEED_U2_ONE, 0]
    return np.concatenate([np.array(special, dtype=U), rng.integers(0, 1 << 32, 64 - len(special), dtype=np.uint64).astype(U)])


def surface_inputs(rng, sampler):
    return surface_bulk(rng), surface_edges(sampler_seeds(rng) if sampler else (1,))


# ---------------------------------------------------------------------------------------------- ReSTIR DI reservoir update
def di_inputs(rng):
    cand = rng.integers(0, 1 << 32, BULK, dtype=np.uint64).astype(U)
    w = rng.uniform(0.0, 10.0, BULK).astype(F)
    pdf = (1.0 - rng.uniform(0.0, 1.0, BULK)).astype(F)                                       # (0, 1]
    seed = rng.integers(0, 1 << 32, BULK, dtype=np.uint64).astype(U)
    bulk = rows(cand, w, pdf, seed)
    e = [(7, wv, pv, sv) for wv, pv, sv in itertools.product([0.0, -0.0, float(DENORM_MIN), float(INF), float(NAN), -1.0, 1.0, 3.0e38],
                                                             [0.0, float(NAN), 0.5, 1.0], [0, 1, SEED_U_ZERO, SEED_U_BELOW_ONE, SEED_U_ONE, 0xFFFFFFFF])]
    e = np.array(e, dtype=np.float64)
    return bulk, rows(e[:, 0].astype(U), e[:, 1].astype(F), e[:, 2].astype(F), e[:, 3].astype(U))


# ---------------------------------------------------------------------------------------------- textures
TEXTURE_SHAPES = [(1, 1), (1, 7), (7, 1), (2, 2), (5, 3), (16, 24)]      # width x height


def textures(rng):
    return [rng.integers(0, 1 << 32, (h, w), dtype=np.uint64).astype(U) for w, h in TEXTURE_SHAPES]


def albedo_inputs(rng):
    uv = rng.uniform(-0.25, 1.25, (BULK, 2)).astype(F)
    bulk = rows(uv, rng.integers(0, len(TEXTURE_SHAPES), BULK).astype(U))
    one = F(1)
    vals = [-0.0, 0.0, 1.0, np.nextafter(one, F(0)), np.nextafter(one, F(2)), 2.0, -1.0, NAN, INF, -INF, 0.37]
    for d in sorted({s - 1 for wh in TEXTURE_SHAPES for s in wh if s > 1}):                   # k / (w - 1): x lands on a texel exactly
        vals += [F(k) / F(d) for k in range(1, d)]
    vals = np.array(vals, dtype=F)
    uu, vv, tt = np.meshgrid(vals, vals, np.arange(len(TEXTURE_SHAPES)), indexing="ij")
    return bulk, rows(uu.ravel().astype(F), vv.ravel().astype(F), tt.ravel().astype(U))


def unpack_word_rgb(words):
    """the oracle's SampleBilinear word as sample_albedo returns it: rgb of UnpackABGR"""
    w = np.asarray(words, dtype=U).reshape(-1)
    k = F(1.0) / F(255.0)
    return np.stack([(w & U(0xFF)).astype(F) * k, ((w >> U(8)) & U(0xFF)).astype(F) * k, ((w >> U(16)) & U(0xFF)).astype(F) * k], axis=1)


# ---------------------------------------------------------------------------------------------- light-tree cluster importance
def cluster_rows(sp, energy, axis, theta_o, theta_e, lo, hi, centroid):
    n = len(sp)
    z = np.zeros(n, dtype=U)
    return rows(np.asarray(sp, dtype=F), np.asarray(energy, dtype=F), z, z, z, z, np.asarray(axis, dtype=F), np.asarray(theta_o, dtype=F),
                np.asarray(theta_e, dtype=F), np.asarray(lo, dtype=F), np.asarray(hi, dtype=F), np.asarray(centroid, dtype=F), z)


def cluster_bulk(rng, n=BULK, flat=None):
    """random boxes (`flat`: no extent along that axis, same bits in lo and hi), unit cone axes, shading points around the box"""
    lo = rng.uniform(-5.0, 5.0, (n, 3)).astype(F)
    ext = rng.uniform(0.0, 3.0, (n, 3)).astype(F)
    if flat is not None:
        ext[:, flat] = 0
    hi = lo + ext
    centroid = (lo + hi) * F(0.5)                                                            # AABB::FindCentroid
    d = unit_vectors(rng, n) * rng.uniform(0.05, 20.0, (n, 1)).astype(F)
    sp = centroid + d.astype(F)
    return cluster_rows(sp, rng.uniform(0.0, 10.0, n), unit_vectors(rng, n), rng.uniform(0.0, np.pi / 2, n), rng.uniform(0.0, np.pi / 2, n), lo, hi, centroid)


def cluster_edges(flat=None):
    """`flat` = None: every box; 0 / 1 / 2: only the boxes without extent along that axis (a whole call of them takes the variant for it)"""
    boxes = [((-1.0, 0.5, 2.0), (1.5, 1.75, 2.5)),                                            # regular
             ((0.25, 0.5, -1.0), (0.25, 0.5, -1.0)),                                           # a point
             ((0.25, 0.5, -1.0), (2.25, 0.5, -1.0)), ((0.25, 0.5, -1.0), (0.25, 1.5, -1.0)), ((0.25, 0.5, -1.0), (0.25, 0.5, 3.0)),   # lines
             ((0.0, 0.5, -1.0), (0.0, 2.5, 1.0)), ((-1.0, 2.0, -1.0), (1.0, 2.0, 3.0)), ((-1.0, 0.0, 0.5), (1.0, 4.0, 0.5))]           # planes x, y, z
    recs = []
    for lo, hi in boxes:
        lo, hi = np.array(lo, dtype=F), np.array(hi, dtype=F)
        if flat is not None and lo[flat] != hi[flat]:
            continue
        c = (lo + hi) * F(0.5)
        diam = float(np.linalg.norm((hi - lo).astype(np.float64))) or 1.0
        face = c.copy(); face[1] = hi[1]
        pts = [c,                                                                              # at the centre (normalize(0))
               (lo * F(0.75) + hi * F(0.25)).astype(F),                                        # inside
               face, hi, lo,                                                                   # on a face, at two corners
               (hi + np.array([0.5, 0.25, 1.0], dtype=F)).astype(F),                            # outside, near
               (c + np.array([0.6, -0.64, 0.48], dtype=F) * F(1.0e4 * diam)).astype(F)]         # 10^4 box diameters away
        for p, th_o, energy, axis in itertools.product(pts, (0.0, float(KPI) / 2, float(KPI)), (0.0, 2.5), ((0.0, -1.0, 0.0), (0.0, 0.0, 0.0), (0.6, 0.0, 0.8))):
            recs.append((p, energy, axis, th_o, float(KPI) / 2, lo, hi, c))
    cols = list(zip(*recs))
    return cluster_rows(np.array(cols[0]), cols[1], np.array(cols[2]), cols[3], cols[4], np.array(cols[5]), np.array(cols[6]), np.array(cols[7]))


# ---------------------------------------------------------------------------------------------- the probes of the test modules
# name -> (probe, function of a Generator giving (bulk, edges)); PROBE_SAMPLE_ALBEDO and the flat-box cluster runs are set up by the tests
PROBES = {
    "sincos_f": (capi.PROBE_SINCOS, sincos_inputs),
    "acos_f": (capi.PROBE_ACOS, acos_inputs),
    "asin_kernel": (capi.PROBE_ASIN_KERNEL, asin_kernel_inputs),
    "pow5_f": (capi.PROBE_POW5, pow5_inputs),
    "rnd": (capi.PROBE_RND, rnd_inputs),
    "oct_encode": (capi.PROBE_OCT_ENCODE, oct_encode_inputs),
    "oct_decode": (capi.PROBE_OCT_DECODE, oct_decode_inputs),
    "pack_abgr": (capi.PROBE_PACK_ABGR, pack_inputs),
    "unpack_abgr": (capi.PROBE_UNPACK_ABGR, unpack_inputs),
    "eval_brdf": (capi.PROBE_EVAL_BRDF, lambda rng: surface_inputs(rng, False)),
    "pdf_brdf": (capi.PROBE_PDF_BRDF, lambda rng: surface_inputs(rng, False)),
    "pdf_ggx": (capi.PROBE_PDF_GGX, lambda rng: surface_inputs(rng, False)),
    "sample_uniform": (capi.PROBE_SAMPLE_UNIFORM, lambda rng: surface_inputs(rng, True)),
    "sample_cosine": (capi.PROBE_SAMPLE_COSINE, lambda rng: surface_inputs(rng, True)),
    "sample_ggx": (capi.PROBE_SAMPLE_GGX, lambda rng: surface_inputs(rng, True)),
    "sample_brdf": (capi.PROBE_SAMPLE_BRDF, lambda rng: surface_inputs(rng, True)),
    "di_update": (capi.PROBE_DI_UPDATE, di_inputs),
    "cluster_importance": (capi.PROBE_CLUSTER_IMPORTANCE, lambda rng: (cluster_bulk(rng), cluster_edges())),
    "cluster_importance_general": (capi.PROBE_CLUSTER_IMPORTANCE_GENERAL, lambda rng: (cluster_bulk(rng), cluster_edges())),
}
SEED = 20261019


def rng_for(name):
    return np.random.default_rng([SEED, sum(name.encode())])


# output words that hold a binary32 (the others are integers: seeds, packed colours, counts, flags)
FLOAT_COLS = {capi.PROBE_SINCOS: (0, 1), capi.PROBE_ACOS: (0,), capi.PROBE_POW5: (0,), capi.PROBE_RND: (0,), capi.PROBE_OCT_ENCODE: (0, 1),
              capi.PROBE_OCT_DECODE: (0, 1, 2), capi.PROBE_PACK_ABGR: (), capi.PROBE_UNPACK_ABGR: (0, 1, 2, 3), capi.PROBE_EVAL_BRDF: (0, 1, 2),
              capi.PROBE_PDF_BRDF: (0,), capi.PROBE_PDF_GGX: (0,), capi.PROBE_SAMPLE_UNIFORM: (0, 1, 2, 3), capi.PROBE_SAMPLE_COSINE: (0, 1, 2, 3),
              capi.PROBE_SAMPLE_GGX: (0, 1, 2, 3), capi.PROBE_SAMPLE_BRDF: (0, 1, 2, 3), capi.PROBE_DI_UPDATE: (1, 2, 3), capi.PROBE_SAMPLE_ALBEDO: (0, 1, 2),
              capi.PROBE_CLUSTER_IMPORTANCE: (0,), capi.PROBE_CLUSTER_IMPORTANCE_GENERAL: (0,),
              capi.PROBE_ASIN_KERNEL: ()}      # (one binary64: its arguments give no NaN, so its two words are compared as they are)


def nan_words(probe, out):
    """(count, words) mask: output words that are a binary32 NaN"""
    m = np.zeros(out.shape, dtype=bool)
    cols = list(FLOAT_COLS[probe])
    if cols:
        m[:, cols] = np.isnan(out[:, cols].view(F))
    return m


def nan_share(probe, out):
    """share of the records with a NaN in any output component"""
    return float(nan_words(probe, out).any(axis=1).mean()) if len(out) else 0.0


def distinct_outputs(out, enough=1000):
    """number of different result records — counted on the first 2^14 records when those already hold `enough` (a lower bound then)"""
    head = len(np.unique(out[:1 << 14], axis=0))
    return head if head >= enough or len(out) <= 1 << 14 else len(np.unique(out, axis=0))


def check_non_vacuous(name, probe, ref_bulk):
    """conditions on a bulk array, computed on the ORACLE's outputs only: few NaNs, many different results"""
    share, distinct = nan_share(probe, ref_bulk), distinct_outputs(ref_bulk)
    assert share <= 0.05, f"{name}: {share:.3%} of the bulk records give NaN (at most 5 %)"
    assert distinct >= 1000, f"{name}: only {distinct} distinct bulk results (at least 1000)"
    return share, distinct


def assert_same_bits(name, probe, inputs, dev, ref):
    """device words against oracle words, bit for bit; two NaNs are equal whatever their sign or payload"""
    assert dev.shape == ref.shape, (name, dev.shape, ref.shape)
    same = (dev == ref) | (nan_words(probe, dev) & nan_words(probe, ref))
    bad = np.flatnonzero(~same.all(axis=1))
    if len(bad):
        i = int(bad[0])
        as_float = inputs[i].view(F).tolist()
        raise AssertionError(f"{name}: {len(bad)} of {len(dev)} records differ; first at index {i}: input words {[hex(int(x)) for x in inputs[i]]} "
                             f"(as binary32 {as_float}); device {[hex(int(x)) for x in dev[i]]}, oracle {[hex(int(x)) for x in ref[i]]}")
    return len(bad)
