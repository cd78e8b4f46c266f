"""Brute-force reference of the batched ray queries (fyprt_trace_rays): the product's ray/triangle test (rt_device.h tri_test, the
reference's Möller–Trumbore, Renderer.cu:513-537) restated in numpy float32 over EVERY leaf record of ctx.export_bvh() — no tree, so
it shows what a traversal must find.  Same operation order as the device (cross = a.y*b.z - b.y*a.z, ...; dot = (x + y) + z; f = 1/det)
and float32 constants throughout, so nothing is promoted to float64 and every accepted t is the device's bit for bit.
A helper of the query tests, not a test file."""
import numpy as np

F32 = np.float32
EPS = np.float32(1e-4)
FLT_MAX = np.float32(3.402823466e38)
ONE, ZERO = np.float32(1.0), np.float32(0.0)


def leaf_records(bvh):
    """(v0, e1, e2, triangle index) of the exported leaf records, float32 (T, 3) each."""
    t = bvh["tris"]
    return (np.ascontiguousarray(t["v0"], F32), np.ascontiguousarray(t["e1"], F32), np.ascontiguousarray(t["e2"], F32),
            t["tri"].astype(np.int64))


def _cross(a, b):
    return (a[1] * b[2] - b[1] * a[2], a[2] * b[0] - b[2] * a[0], a[0] * b[1] - b[0] * a[1])


def _dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def tri_test(o, d, v0, e1, e2):
    """tri_test for rays (R, 3) x triangles (T, 3): (passes, t) as (R, T) arrays (t is meaningful where it passes)."""
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
    return ok, t


def _batches(n, size):
    for b in range(0, n, size):
        yield slice(b, min(n, b + size))


def _interval(x, n):
    return np.broadcast_to(np.asarray(x, dtype=F32), (n,))


def closest(bvh, o, d, tmin=0.0, tmax=np.inf, batch=64):
    """Closest accepted triangle per ray: (t, triangle, ties) — t float32 (-1 where nothing is accepted), triangle int64 (-1), ties a list
    of the triangle sets accepted at exactly that t (any of them is a valid answer: which one a traversal finds first depends on its order).
    Accepted: tri_test passes, t > tmin, t < min(tmax, FLT_MAX)."""
    v0, e1, e2, ids = leaf_records(bvh)
    o, d = np.asarray(o, F32).reshape(-1, 3), np.asarray(d, F32).reshape(-1, 3)
    n = len(o)
    lo, hi = _interval(tmin, n), np.minimum(_interval(tmax, n), FLT_MAX)
    best = np.full(n, -1.0, dtype=F32)
    tri = np.full(n, -1, dtype=np.int64)
    ties = [frozenset()] * n
    for sl in _batches(n, batch):
        ok, t = tri_test(o[sl], d[sl], v0, e1, e2)
        with np.errstate(invalid="ignore"):
            ok &= (t > lo[sl, None]) & (t < hi[sl, None])
        tm = np.where(ok, t, np.inf).astype(F32)
        m = tm.min(axis=1)
        for r in np.nonzero(np.isfinite(m))[0]:
            tied = ids[tm[r] == m[r]]
            best[sl.start + r], tri[sl.start + r], ties[sl.start + r] = m[r], tied[0], frozenset(tied.tolist())
    return best, tri, ties


def occluded(bvh, o, d, tmin, tmax, batch=64):
    """Any accepted triangle per ray (tri_test passes, tmin < t < tmax): bool (R,)."""
    v0, e1, e2, _ = leaf_records(bvh)
    o, d = np.asarray(o, F32).reshape(-1, 3), np.asarray(d, F32).reshape(-1, 3)
    n = len(o)
    lo, hi = _interval(tmin, n), _interval(tmax, n)
    out = np.zeros(n, dtype=bool)
    for sl in _batches(n, batch):
        ok, t = tri_test(o[sl], d[sl], v0, e1, e2)
        with np.errstate(invalid="ignore"):
            out[sl] = (ok & (t > lo[sl, None]) & (t < hi[sl, None])).any(axis=1)
    return out


def random_rays(scene, n, seed):
    """n rays from points inside the scene's bounding box (slightly enlarged) in uniformly random directions, float32."""
    rng = np.random.default_rng(seed)
    p = scene.world_vertices["position"].astype(np.float64)
    lo, hi = p.min(axis=0), p.max(axis=0)
    pad = 0.05 * (hi - lo)
    o = rng.uniform(lo - pad, hi + pad, size=(n, 3)).astype(F32)
    d = rng.normal(size=(n, 3))
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(F32)
    return o, d


def check_closest(payload, best, ties):
    """Indices of the rays where a closest-hit payload disagrees with the brute force: hitDistance bit for bit, objectIndex in the
    tie set, a miss (-1, -1) exactly where nothing is accepted."""
    hd = payload["hitDistance"].astype(F32)
    obj = payload["objectIndex"]
    bad = []
    for i in range(len(payload)):
        if best[i] < 0:
            ok = hd[i] == F32(-1.0) and obj[i] == -1
        else:
            ok = hd[i].view(np.uint32) == best[i].view(np.uint32) and int(obj[i]) in ties[i]
        if not ok:
            bad.append(i)
    return bad
