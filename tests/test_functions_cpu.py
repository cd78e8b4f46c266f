"""CPU-side tests of the per-function probes: the new entry point's argument and state checks on a host-only context,
the oracle's array entry point against its scalar hooks, the non-vacuity of the argument sets tests/test_gpu_functions.py sends to
the device, and the oracle's new pdf / cluster-importance exports against an independent float64 transcription of the reference's
formulas.  No GPU."""
import ctypes as C

import numpy as np
import pytest

import function_probes as fp
import oraclelib
from fypraytracer_amd import capi, scenes

F, U = np.float32, np.uint32


def test_selftest_functions_argument_and_state_checks_on_a_host_only_context():
    ctx = capi.Context(-1)
    lib, x, out = ctx.lib, np.zeros((4, 1), dtype=F), np.zeros((4, 2), dtype=U)
    call = lambda probe, i, n, o: lib.fyprt_selftest_functions(ctx.h, probe, None if i is None else i.ctypes.data, n, None if o is None else o.ctypes.data)
    EINVAL, ESTATE = -1, -3
    assert call(-1, x, 4, out) == EINVAL and call(capi.PROBE_ASIN_KERNEL + 1, x, 4, out) == EINVAL      # unknown probe
    assert b"unknown probe" in lib.fyprt_last_error(ctx.h)
    assert call(capi.PROBE_SINCOS, None, 4, out) == EINVAL and call(capi.PROBE_SINCOS, x, 4, None) == EINVAL            # NULL records, count > 0
    assert lib.fyprt_selftest_functions(None, 0, x.ctypes.data, 4, out.ctypes.data) == EINVAL                          # NULL context
    assert call(capi.PROBE_SINCOS, x, 4, out) == ESTATE                                                                 # valid arguments: no device
    assert call(capi.PROBE_SINCOS, None, 0, None) == ESTATE
    assert b"needs a device" in lib.fyprt_last_error(ctx.h)
    ctx.upload_scene(scenes.cornell_box())
    assert call(capi.PROBE_SAMPLE_ALBEDO, np.zeros((1, 3), dtype=F), 1, np.zeros((1, 3), dtype=U)) == ESTATE
    with pytest.raises(capi.FyprtError, match="needs a device"):
        ctx.selftest_functions(capi.PROBE_ACOS, x)
    with pytest.raises(capi.FyprtError, match="unknown probe"):
        ctx.selftest_functions(99, x)
    assert (out == 0).all() and capi.live_device_bytes() == 0
    ctx.close()
    assert len(capi.PROBE_IN_WORDS) == len(capi.PROBE_OUT_WORDS) == len(fp.FLOAT_COLS) == capi.PROBE_ASIN_KERNEL + 1


def test_pcg_unhash_gives_the_seeds_that_draw_zero_and_one(oracle_built):
    lib = oraclelib.lib()
    for h in (0, 1, 0xFFFFFF7F, 0xFFFFFF80, 0xFFFFFFFF, 0x12345678, 0x9E3779B9):
        assert fp.pcg_hash(fp.pcg_unhash(h)) == h and lib.orc_pcg_hash(fp.pcg_unhash(h)) == h
    draw = lambda s: (lambda c: (lib.orc_random_float(C.byref(c)), c.value))(C.c_uint32(s))
    assert draw(fp.SEED_U_ZERO) == (0.0, 0) and draw(fp.SEED_U_ONE) == (1.0, 0xFFFFFF80) and draw(fp.SEED_U_ONE_MAX)[0] == 1.0
    assert draw(fp.SEED_U_BELOW_ONE)[0] == float(np.nextafter(F(1), F(0)))
    assert draw(fp.SEED_U2_ZERO)[1] == fp.SEED_U_ZERO and draw(fp.SEED_U2_ONE)[1] == fp.SEED_U_ONE


def _scalar(lib, probe, w, textures):
    """one record through the oracle's scalar hooks -> result words"""
    f = w.view(F)
    p = lambda a: np.ascontiguousarray(a).ctypes.data
    o = np.zeros(capi.PROBE_OUT_WORDS[probe] if probe != capi.PROBE_SAMPLE_ALBEDO else 1, dtype=U)
    g = o.view(F)
    if probe == capi.PROBE_SINCOS: g[0], g[1] = lib.orc_sin(f[0]), lib.orc_cos(f[0])
    elif probe == capi.PROBE_ACOS: g[0] = lib.orc_acos(f[0])
    elif probe == capi.PROBE_POW5: g[0] = lib.orc_pow5(f[0])
    elif probe == capi.PROBE_RND:
        s = C.c_uint32(int(w[0])); g[0] = lib.orc_random_float(C.byref(s)); o[1] = s.value
    elif probe == capi.PROBE_OCT_ENCODE: lib.orc_encode_oct(p(f), o.ctypes.data)
    elif probe == capi.PROBE_OCT_DECODE: lib.orc_decode_oct(p(f), o.ctypes.data)
    elif probe == capi.PROBE_PACK_ABGR: o[0] = lib.orc_convert_rgba(p(f))
    elif probe == capi.PROBE_UNPACK_ABGR: lib.orc_unpack_abgr(int(w[0]), o.ctypes.data)
    elif probe == capi.PROBE_EVAL_BRDF: lib.orc_brdf(p(f[0:3]), p(f[3:6]), p(f[6:9]), p(f[9:12]), f[12], f[13], o.ctypes.data)
    elif probe == capi.PROBE_PDF_BRDF: g[0] = lib.orc_pdf_brdf(p(f[0:3]), p(f[3:6]), p(f[6:9]), p(f[9:12]), f[12], f[13])
    elif probe == capi.PROBE_PDF_GGX: g[0] = lib.orc_pdf_ggx(p(f[0:3]), p(f[3:6]), p(f[6:9]), f[13])
    elif capi.PROBE_SAMPLE_UNIFORM <= probe <= capi.PROBE_SAMPLE_BRDF:
        s = C.c_uint32(int(w[14]))
        lib.orc_sample(probe - capi.PROBE_SAMPLE_UNIFORM, p(f[0:3]), p(f[3:6]), p(f[9:12]), f[12], f[13], C.byref(s), o.ctypes.data); o[4] = s.value
    elif probe == capi.PROBE_DI_UPDATE:
        s, acc = C.c_uint32(int(w[3])), C.c_int(0)
        lib.orc_di_reset_update(int(w[0]), f[1], f[2], C.byref(s), o.ctypes.data, C.byref(acc)); o[5], o[6] = acc.value, s.value
    elif probe == capi.PROBE_SAMPLE_ALBEDO:
        t = textures[int(w[2])]
        o[0] = lib.orc_sample_bilinear(t.ctypes.data, t.shape[1], t.shape[0], f[0], f[1])
    elif probe == capi.PROBE_ASIN_KERNEL: o.view(np.float64)[0] = lib.orc_asin_kernel(float(w.view(np.float64)[0]))
    else: g[0] = lib.orc_cluster_importance(p(f[0:3]), p(w[3:23]))
    return o


@pytest.fixture(scope="module")
def oracle_outputs(oracle_built):
    """the oracle's result words for every probe's (bulk, edges), computed once"""
    out = {}
    for name, (probe, gen) in fp.PROBES.items():
        bulk, edge = gen(fp.rng_for(name))
        out[name] = (probe, bulk, edge, oraclelib.probe(probe, bulk), oraclelib.probe(probe, edge), ())
    rng = fp.rng_for("sample_albedo")
    tex = fp.textures(rng)
    bulk, edge = fp.albedo_inputs(rng)
    out["sample_albedo"] = (capi.PROBE_SAMPLE_ALBEDO, bulk, edge, oraclelib.probe(capi.PROBE_SAMPLE_ALBEDO, bulk, tex), oraclelib.probe(capi.PROBE_SAMPLE_ALBEDO, edge, tex), tex)
    return out


@pytest.mark.parametrize("name", list(fp.PROBES) + ["sample_albedo"])
def test_oracle_array_form_equals_its_scalar_hooks_and_the_bulk_is_not_vacuous(oracle_outputs, name):
    probe, bulk, edge, ref_bulk, ref_edge, tex = oracle_outputs[name]
    lib = oraclelib.lib()
    step = max(1, len(edge) // 256)
    for inputs, ref in ((bulk[:128], ref_bulk[:128]), (edge[::step], ref_edge[::step])):
        one = np.array([_scalar(lib, probe, w, tex) for w in inputs])
        same = (one == ref) | (np.isnan(one.view(F)) & np.isnan(ref.view(F)) & (fp.nan_words(probe, ref) if probe != capi.PROBE_SAMPLE_ALBEDO else False))
        assert same.all(), (name, np.flatnonzero(~same.all(axis=1))[:4])
    if probe == capi.PROBE_SAMPLE_ALBEDO:
        ref_bulk = fp.unpack_word_rgb(ref_bulk).view(U)
    fp.check_non_vacuous(name, probe, ref_bulk)


def test_flat_box_bulks_are_not_vacuous(oracle_built):
    for axis in range(3):
        bulk = fp.cluster_bulk(fp.rng_for(f"flat{axis}"), 1 << 16, flat=axis)
        assert (bulk[:, 13 + axis] == bulk[:, 16 + axis]).all() and len(fp.cluster_edges(flat=axis)) % 126 == 0 and len(fp.cluster_edges(flat=axis)) > 0
        fp.check_non_vacuous(f"flat{axis}", capi.PROBE_CLUSTER_IMPORTANCE, oraclelib.probe(capi.PROBE_CLUSTER_IMPORTANCE, bulk))


def test_bilinear_sample_with_nan_uv_is_defined(oracle_built):
    """(int)NaN is undefined in C++ (x86 gives INT_MIN: a texel index far outside the texture).  Oracle and device convert NaN to 0:
    the four texels read are in range, the interpolation weights are NaN, and a NaN colour packs to 0"""
    lib = oraclelib.lib()
    for t in fp.textures(fp.rng_for("sample_albedo")):
        s = lambda u, v: lib.orc_sample_bilinear(t.ctypes.data, t.shape[1], t.shape[0], F(u), F(v))
        assert s(np.nan, np.nan) == 0 and s(np.nan, 1.0) == 0 and s(0.5, np.nan) == 0


# ---------------------------------------------------------------------------------------------- float64 transcriptions
def _dot(a, b):
    return np.sum(a * b, axis=-1)


def _normalize(a):
    return a / np.sqrt(_dot(a, a))[..., None]


PI32 = float(F(3.1415926535))          # MathUtils.cuh:17 `pi` as the binary32 the reference uses


def ggx_pdf64(N, V, L, roughness):      # MathUtils.cuh:176-190
    H = _normalize(V + L)
    NdotH, VdotH = np.maximum(_dot(N, H), 0.0), np.maximum(_dot(V, H), 0.0)
    a2 = (roughness * roughness) ** 2
    denom = NdotH * NdotH * (a2 - 1.0) + 1.0
    with np.errstate(all="ignore"):
        pdf = (a2 / (PI32 * denom * denom)) * NdotH / (4.0 * VdotH)
    return np.where((NdotH <= 0.0) | (VdotH <= 0.0), 0.0, pdf)


def brdf_pdf64(N, V, L, albedo, metallic, roughness):      # MathUtils.cuh:246-274
    spec, diff = ggx_pdf64(N, V, L, roughness), np.maximum(_dot(N, L), 0.0) / PI32
    F0 = float(F(0.04)) * (1.0 - metallic)[:, None] + albedo * metallic[:, None]
    Fr = F0 + (1.0 - F0) * ((1.0 - np.maximum(_dot(N, V), 0.0)) ** 5)[:, None]
    w = Fr.sum(axis=1) / 3.0
    return np.where(metallic == 1.0, spec, np.where(metallic == 0.0, diff, w * spec + (1.0 - w) * diff))


def cluster_importance64(sp, energy, axis, theta_o, theta_e, lo, hi, centroid):      # LightTree.cuh:91-117, ConeBounds.cuh:47-87
    cone_axis = _normalize(centroid - sp)
    theta_u = np.zeros(len(sp))
    for k in range(8):
        corner = np.stack([np.where(k & 4, hi[:, 0], lo[:, 0]), np.where(k & 2, hi[:, 1], lo[:, 1]), np.where(k & 1, hi[:, 2], lo[:, 2])], axis=1)
        theta_u = np.maximum(theta_u, np.arccos(np.clip(_dot(cone_axis, _normalize(corner - sp)), -1.0, 1.0)))
    d = sp - centroid
    d2 = np.maximum(_dot(d, d), 1e-12)
    theta = np.arccos(np.clip(_dot(axis, _normalize(d)), -1.0, 1.0))
    angle = np.clip(theta - theta_o - theta_u, 0.0, theta_e)
    return energy * np.cos(angle) / d2, theta_u, theta


MEASURED = {}


def test_new_oracle_exports_agree_with_a_float64_transcription_of_the_reference(oracle_built):
    """orc_pdf_ggx, orc_pdf_brdf and orc_cluster_importance (binary32, the oracle's operation order) against the reference's formulas
    evaluated in float64 numpy, on 2^16 well-conditioned random arguments each: roughness in [0.1, 1]; N.V, N.L, V.H and N.H at least 0.2;
    N.H at most 0.95 (the GGX denominator (N.H)^2 (a^2 - 1) + 1 cancels as H approaches N at a small a^2: at N.H = 0.95 it still keeps
    0.0975 of the 1 it is subtracted from); the shading point 1 to 4 box diagonals from the box centre and outside the box, every cosine that goes through acos at most 0.98 in
    magnitude (acos turns a binary32 rounding error eps of a cosine c into eps / sqrt(1 - c^2)), theta_e at most 1.2 (cos of the angle
    term stays above 0.36).
    Largest relative error measured (x86-64, glibc, numpy 2): pdf_ggx 5.55e-6, pdf_brdf 5.46e-6, cluster importance 1.76e-6.
    Bounds, x4 for other libm / numpy builds and summation orders: 2.3e-5, 2.2e-5 and 7.1e-6."""
    n = 1 << 16
    rng = np.random.default_rng(fp.SEED)
    rec = fp.surface_bulk(rng, 8 * n)
    f = np.ascontiguousarray(rec[:, :14]).view(F).astype(np.float64)
    N, V, L, albedo, metallic = f[:, 0:3], f[:, 3:6], f[:, 6:9], f[:, 9:12], f[:, 12]
    H = _normalize(V + L)
    ok = (_dot(N, V) >= 0.2) & (_dot(N, L) >= 0.2) & (_dot(V, H) >= 0.2) & (_dot(N, H) >= 0.2) & (_dot(N, H) <= 0.95)
    rec = rec[ok][:n].copy()
    assert len(rec) == n
    rec[:, 13] = rng.uniform(0.1, 1.0, n).astype(F).view(U)
    f = np.ascontiguousarray(rec[:, :14]).view(F).astype(np.float64)
    N, V, L, albedo, metallic, roughness = f[:, 0:3], f[:, 3:6], f[:, 6:9], f[:, 9:12], f[:, 12], f[:, 13]

    def rel(got, want):
        return float(np.max(np.abs(got.astype(np.float64) - want) / np.abs(want)))
    MEASURED["pdf_ggx"] = rel(oraclelib.probe(capi.PROBE_PDF_GGX, rec).view(F)[:, 0], ggx_pdf64(N, V, L, roughness))
    MEASURED["pdf_brdf"] = rel(oraclelib.probe(capi.PROBE_PDF_BRDF, rec).view(F)[:, 0], brdf_pdf64(N, V, L, albedo, metallic, roughness))

    m = 8 * n
    lo = rng.uniform(-5.0, 5.0, (m, 3)).astype(F)
    hi = lo + rng.uniform(0.5, 3.0, (m, 3)).astype(F)
    centroid = (lo + hi) * F(0.5)
    diag = np.linalg.norm((hi - lo).astype(np.float64), axis=1, keepdims=True)
    sp = (centroid + fp.unit_vectors(rng, m) * (diag * rng.uniform(1.0, 4.0, (m, 1))).astype(F)).astype(F)
    args = [sp, rng.uniform(0.5, 10.0, m).astype(F), fp.unit_vectors(rng, m), rng.uniform(0.0, 0.5, m).astype(F), rng.uniform(0.2, 1.2, m).astype(F), lo, hi, centroid]
    a64 = [np.asarray(a, dtype=np.float64) for a in args]
    want, theta_u, theta = cluster_importance64(*a64)
    ok = (np.cos(theta_u) <= 0.98) & (np.abs(np.cos(theta)) <= 0.98) & ((a64[0] < a64[5]) | (a64[0] > a64[6])).any(axis=1)
    args = [a[ok][:n] for a in args]
    assert len(args[0]) == n
    want = want[ok][:n]
    MEASURED["cluster_importance"] = rel(oraclelib.probe(capi.PROBE_CLUSTER_IMPORTANCE_GENERAL, fp.cluster_rows(*args)).view(F)[:, 0], want)
    print("largest relative errors against float64:", MEASURED)
    assert MEASURED["pdf_ggx"] <= 2.3e-5 and MEASURED["pdf_brdf"] <= 2.2e-5 and MEASURED["cluster_importance"] <= 7.1e-6, MEASURED
