"""The arithmetic contract function by function: every shading function of the device — evaluated by
fyprt_selftest_functions through the inline functions the frame kernels call — against the CPU oracle's function, BIT FOR BIT, on a
seeded bulk array and an explicit list of edge arguments each (tests/function_probes.py).  One relaxation: two NaNs are equal
whatever their sign or payload (x86 and the GPU produce different default NaNs).  A failure names the probe, the index and input of
the first mismatch and both result records in hex.
sincos_f is fed only what the renderer can reach, 2.0f * kPi * u with u in [0, 1] and the floats around k*pi/2 up to 2*pi: its header
says it is not valid for negative or huge angles."""
import numpy as np
import pytest

import function_probes as fp
import oraclelib
from fypraytracer_amd import capi, scenes

pytestmark = pytest.mark.gpu
F, U = np.float32, np.uint32


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


def run_both(ctx, name, probe, inputs, textures=()):
    dev = ctx.selftest_functions(probe, inputs)
    ref = oraclelib.probe(probe, inputs, textures)
    if probe == capi.PROBE_SAMPLE_ALBEDO:                         # SampleBilinear's word, unpacked as np.float32(byte) * np.float32(1 / 255)
        ref = fp.unpack_word_rgb(ref).view(U)
    print(f"{name}: {len(inputs)} records, {fp.nan_share(probe, ref):.4%} NaN results in the oracle")
    fp.assert_same_bits(name, probe, inputs, dev, ref)
    return ref


@pytest.mark.parametrize("name", list(fp.PROBES))
def test_device_function_equals_oracle_bit_for_bit(ctx, oracle_built, name):
    probe, gen = fp.PROBES[name]
    bulk, edge = gen(fp.rng_for(name))
    assert len(bulk) <= 1 << 20
    run_both(ctx, name + " (edges)", probe, edge)
    ref = run_both(ctx, name + " (bulk)", probe, bulk)
    fp.check_non_vacuous(name, probe, ref)


def test_cluster_importance_flat_box_variants_equal_oracle(ctx, oracle_built):
    """every record of a call flat along one axis: each wave takes cluster_importance's variant for that axis (y before x before z)"""
    for axis in range(3):
        name = f"cluster_importance, boxes flat along axis {axis}"
        run_both(ctx, name + " (edges)", capi.PROBE_CLUSTER_IMPORTANCE, fp.cluster_edges(flat=axis))
        ref = run_both(ctx, name + " (bulk)", capi.PROBE_CLUSTER_IMPORTANCE, fp.cluster_bulk(fp.rng_for(f"flat{axis}"), 1 << 16, flat=axis))
        fp.check_non_vacuous(name, capi.PROBE_CLUSTER_IMPORTANCE, ref)


def test_sample_albedo_equals_oracle_bit_for_bit(oracle_built):
    """textures 1x1, 1x7, 7x1, 2x2, 5x3 and 16x24 — three uploaded with the scene, three appended; NaN and infinite uvs included"""
    rng = fp.rng_for("sample_albedo")
    tex = fp.textures(rng)
    bulk, edge = fp.albedo_inputs(rng)
    c = capi.Context(0)
    with pytest.raises(capi.FyprtError, match="before fyprt_upload_scene"):
        c.selftest_functions(capi.PROBE_SAMPLE_ALBEDO, edge[:4])
    sc = scenes.cornell_box()
    sc.textures = tex[:3]
    c.upload_scene(sc)
    c.append_textures(tex[3:])
    run_both(c, "sample_albedo (edges)", capi.PROBE_SAMPLE_ALBEDO, edge, tex)
    ref = run_both(c, "sample_albedo (bulk)", capi.PROBE_SAMPLE_ALBEDO, bulk, tex)
    fp.check_non_vacuous("sample_albedo", capi.PROBE_SAMPLE_ALBEDO, ref)
    past = c.selftest_functions(capi.PROBE_SAMPLE_ALBEDO, fp.rows(np.array([[0.5, 0.5]], dtype=F), np.array([len(tex)], dtype=U)))
    assert (past.view(F) == -1.0).all()                           # an index past the textures: the material's own albedo (the probe's is -1)
    c.close()


def test_selftest_functions_checks_arguments_and_leaves_the_frame_alone(ctx):
    x = np.zeros((3, 1), dtype=F)
    with pytest.raises(capi.FyprtError, match="unknown probe"):
        ctx.selftest_functions(capi.PROBE_ASIN_KERNEL + 1, x)
    assert ctx.lib.fyprt_selftest_functions(ctx.h, capi.PROBE_ACOS, None, 3, None) == -1               # FYPRT_EINVAL
    assert ctx.lib.fyprt_selftest_functions(ctx.h, capi.PROBE_ACOS, None, 0, None) == 0                # count 0: nothing to do
    assert ctx.selftest_functions(capi.PROBE_ACOS, np.zeros((0, 1), dtype=F)).shape == (0, 1)
    W = H = 32
    c = capi.Context(0)
    c.resize(W, H)
    c.upload_scene(scenes.cornell_box())
    c.set_camera(scenes.cornell_camera(W, H))
    st = capi.Settings(technique=capi.RESTIR_DI, use_temporal_reuse=1, use_spatial_reuse=1)
    c.render(st)
    before = [c.read_buffer(b).copy() for b in (capi.BUF_ACCUM, capi.BUF_IMAGE, capi.BUF_DI, capi.BUF_DI_PREV)]
    index = c.frame_index
    for probe in (capi.PROBE_SAMPLE_BRDF, capi.PROBE_DI_UPDATE, capi.PROBE_CLUSTER_IMPORTANCE):
        c.selftest_functions(probe, np.zeros((1000, capi.PROBE_IN_WORDS[probe]), dtype=U))
    after = [c.read_buffer(b) for b in (capi.BUF_ACCUM, capi.BUF_IMAGE, capi.BUF_DI, capi.BUF_DI_PREV)]
    assert c.frame_index == index
    for a, b in zip(before, after):
        assert a.tobytes() == b.tobytes()
    c.close()
