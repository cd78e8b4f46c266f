"""Brute-force reference of the multi-hit query (fyprt_trace_ray_hits): bruteforce.tri_test's arithmetic over EVERY leaf record of
ctx.export_bvh() — no tree — extended to return the barycentrics u and v from the same expressions, then the accepted hits of a ray
sorted by the key (bits(t) << 32) | triangle.  float32 throughout, the device's operation order: every t, u and v is the device's bit
for bit.  A helper of the multi-hit tests, not a test file."""
import numpy as np

import bruteforce
from bruteforce import EPS, F32, FLT_MAX, ONE, ZERO, _cross, _dot
from fypraytracer_amd import capi

UNUSED = np.array([(-1.0, 0xFFFFFFFF, 0.0, 0.0)], dtype=capi.RAY_HIT_DTYPE)[0]


def tri_test_uv(o, d, v0, e1, e2):
    """bruteforce.tri_test with the barycentrics: (passes, t, u, v) as (R, T) arrays."""
    with np.errstate(all="ignore"):
        O = [o[:, k:k + 1].astype(F32) for k in range(3)]
        D = [d[:, k:k + 1].astype(F32) for k in range(3)]
        V0 = [v0[None, :, k] for k in range(3)]
        E1 = [e1[None, :, k] for k in range(3)]
        E2 = [e2[None, :, k] for k in range(3)]
        hh = _cross(D, E2)
        det = _dot(E1, hh)
        f = ONE / det
        s = [O[k] - V0[k] for k in range(3)]
        u = f * _dot(s, hh)
        ok = ~((u < ZERO) | (u > ONE))
        q = _cross(s, E1)
        v = f * _dot(D, q)
        ok &= ~((v < ZERO) | ((u + v) > ONE))
        t = f * _dot(E2, q)
        ok &= t > EPS
    return ok, t, u, v


def hit_keys(rec):
    """The 64-bit order key of hit records: (bits(t) << 32) | triangle."""
    return (np.ascontiguousarray(rec["t"]).view(np.uint32).astype(np.uint64) << np.uint64(32)) | rec["triangle"].astype(np.uint64)


def k_nearest(bvh, o, d, tmin, tmax, k, after=None, batch=64):
    """The k smallest-key accepted hits per ray: (hits (R, k) RAY_HIT_DTYPE, counts (R,) uint32, totals (R,) int64).  Accepted: tri_test
    passes, t > tmin, t < min(tmax, FLT_MAX) and, with `after` (R RAY_HIT_DTYPE records), key > key(after[i]); an after[i] with t < 0
    finishes the ray (nothing accepted).  Unused records are UNUSED; totals counts every accepted hit, also beyond k."""
    v0, e1, e2, ids = bruteforce.leaf_records(bvh)
    o, d = np.asarray(o, F32).reshape(-1, 3), np.asarray(d, F32).reshape(-1, 3)
    n = len(o)
    lo, hi = bruteforce._interval(tmin, n), np.minimum(bruteforce._interval(tmax, n), FLT_MAX)
    hits = np.full((n, k), UNUSED, dtype=capi.RAY_HIT_DTYPE)
    counts = np.zeros(n, dtype=np.uint32)
    totals = np.zeros(n, dtype=np.int64)
    if after is not None:
        after = np.asarray(after).reshape(-1)
        assert after.dtype == capi.RAY_HIT_DTYPE and len(after) == n
        after_key, finished = hit_keys(after), after["t"] < 0
    for sl in bruteforce._batches(n, batch):
        ok, t, u, v = tri_test_uv(o[sl], d[sl], v0, e1, e2)
        with np.errstate(invalid="ignore"):
            ok &= (t > lo[sl, None]) & (t < hi[sl, None])
        for r in range(ok.shape[0]):
            i = sl.start + r
            if after is not None and finished[i]:
                continue
            m = np.nonzero(ok[r])[0]
            tb = np.ascontiguousarray(t[r, m], dtype=F32).view(np.uint32)
            tri = ids[m].astype(np.uint32)
            if after is not None:
                keep = ((tb.astype(np.uint64) << np.uint64(32)) | tri.astype(np.uint64)) > after_key[i]
                m, tb, tri = m[keep], tb[keep], tri[keep]
            order = np.lexsort((tri, tb))                    # primary key: the bits of t; ties: the triangle index
            totals[i] = len(order)
            order = order[:k]
            c = len(order)
            counts[i] = c
            hits["t"][i, :c], hits["triangle"][i, :c] = t[r, m[order]], tri[order]
            hits["u"][i, :c], hits["v"][i, :c] = u[r, m[order]], v[r, m[order]]
    return hits, counts, totals


def all_hits(bvh, o, d, tmin, tmax, batch=64):
    """Every accepted hit per ray in key order, in trace_all_hits' shape: (flat records, offsets (R + 1,) int64)."""
    n = len(np.asarray(o).reshape(-1, 3))
    _, _, totals = k_nearest(bvh, o, d, tmin, tmax, 1, batch=batch)
    kmax = max(1, int(totals.max(initial=0)))
    hits, counts, _ = k_nearest(bvh, o, d, tmin, tmax, kmax, batch=batch)
    offsets = np.concatenate([[0], np.cumsum(counts.astype(np.int64))]).astype(np.int64)
    flat = np.concatenate([hits[i, :counts[i]] for i in range(n)]) if n else np.empty(0, dtype=capi.RAY_HIT_DTYPE)
    return flat, offsets


def records_equal(a, b):
    """Bit-for-bit equality of two arrays of 16-byte hit records."""
    a8, b8 = np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8)
    return a8.shape == b8.shape and bool((a8 == b8).all())


def record_diff(a, b):
    """Indices (first axis) where hit records differ in any bit."""
    a8 = np.ascontiguousarray(a).view(np.uint8).reshape(len(a), -1)
    b8 = np.ascontiguousarray(b).view(np.uint8).reshape(len(b), -1)
    return np.nonzero((a8 != b8).any(axis=1))[0]


def layers_scene():
    """12 parallel quads 0.25 apart (normal +y), 3 of them added a second time as separate meshes: coplanar copies with identical
    vertices, so a ray through one has two hits at exactly the same t on different triangle indices."""
    from fypraytracer_amd.scene import Material, Scene
    from fypraytracer_amd.scenes import _quad
    sc = Scene()
    sc.materials = [Material(albedo=(1, 1, 1), roughness=1.0, metallic=0.0), Material(albedo=(1, 1, 1), emission_color=(1, 1, 1), emission_power=5.0)]

    def layer(j):
        y = -0.25 * j
        h = 1.0 + 0.1 * (j % 4)                              # unequal extents: rays near the rim cross only some layers
        return _quad((-h, y, h), (h, y, h), (h, y, -h), (-h, y, -h), (0, 1, 0))
    for j in range(12):
        sc.add_new_mesh_to_scene(*layer(j), material_index=1 if j == 11 else 0)
    for j in (0, 4, 7):
        sc.add_new_mesh_to_scene(*layer(j), material_index=0)
    sc.init_scene_emissive_triangles()
    return sc


def layers_rays(n=600, seed=11):
    """Jittered origins above the stack, directions within about 20 degrees of -y."""
    rng = np.random.default_rng(seed)
    o = np.stack([rng.uniform(-1.6, 1.6, n), rng.uniform(0.5, 1.0, n), rng.uniform(-1.6, 1.6, n)], 1).astype(F32)
    ang = np.radians(rng.uniform(0.0, 20.0, n))
    phi = rng.uniform(0.0, 2 * np.pi, n)
    d = np.stack([np.sin(ang) * np.cos(phi), -np.cos(ang), np.sin(ang) * np.sin(phi)], 1).astype(F32)
    return o, d
