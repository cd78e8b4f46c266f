"""ctypes binding of the C ABI in include/fyprt.h (libfyprt.so).

The product path has no CPU fallback: if the HIP library is missing or cannot be loaded
this module raises, loudly.  Nothing here imports or touches oracle/.
"""
from __future__ import annotations

import contextlib
import ctypes as C
import os
from pathlib import Path

import numpy as np

_PKG = Path(__file__).resolve().parent
LIB_PATH = _PKG / "csrc" / "libfyprt.so"

# technique ids: SamplingTechniqueEnum.h:4-17
BRUTE_FORCE, UNIFORM_SAMPLING, COSINE_WEIGHTED_SAMPLING, GGX_SAMPLING, BRDF_SAMPLING = 0, 1, 2, 3, 4
LIGHT_SOURCE_SAMPLING, NEE, RESTIR_DI, RESTIR_GI = 5, 6, 7, 8
TECHNIQUE_NAMES = ["BRUTE_FORCE", "UNIFORM_SAMPLING", "COSINE_WEIGHTED_SAMPLING", "GGX_SAMPLING", "BRDF_SAMPLING",
                   "LIGHT_SOURCE_SAMPLING", "NEE", "RESTIR_DI", "RESTIR_GI"]

BUF_ACCUM, BUF_IMAGE, BUF_PAYLOAD, BUF_DEPTH, BUF_NORMAL, BUF_DI, BUF_DI_PREV, BUF_GI, BUF_GI_PREV = range(9)
BUF_TEMPORAL = 10   # 64 B per pixel: the history record the last Context.denoise_temporal* call wrote (TEMPORAL_DTYPE)
BUF_UPSCALE_GUIDE = 11    # 32 B per HI-RES pixel: the guide record of the hi-res primary hit (UPSCALE_GUIDE_DTYPE); Context.denoise_upscale*
BUF_UPSCALE_ALBEDO = 12   # float4 per hi-res pixel: albedo | 1 (filterable) or pass-through colour | 0
BUF_ALBEDO = 9      # float4 per pixel: albedo of the primary hit, w = 1 filterable / 0 not; written by Context.denoise* (fyprt_denoise)

# numpy views of the per-pixel records (Ray.h:13-22, ReSTIR_DI_Reservoir.cuh:9-16, ReSTIR_GI_Reservoir.cuh:9-27)
PAYLOAD_DTYPE = np.dtype([("hitDistance", "<f4"), ("worldPosition", "<f4", 3), ("worldNormal", "<f4", 3),
                          ("u", "<f4"), ("v", "<f4"), ("objectIndex", "<i4")])
DI_DTYPE = np.dtype([("indexEmissive", "<u4"), ("weightEmissive", "<f4"), ("emissivePDF", "<f4"),
                     ("weightSum", "<f4"), ("M", "<u4")])
GI_DTYPE = np.dtype([("visiblePoint", "<f4", 3), ("visibleNormal", "<f4", 2), ("samplePoint", "<f4", 3),
                     ("sampleNormal", "<f4", 2), ("Lo", "<f4", 3), ("randSeed", "<u4"), ("samplePDF", "<f4"),
                     ("weightSample", "<f4"), ("M", "<u4"), ("weightSum", "<f4")])
assert PAYLOAD_DTYPE.itemsize == 40 and DI_DTYPE.itemsize == 20 and GI_DTYPE.itemsize == 72
# the temporal denoiser's history record (include/fyprt.h, "temporal denoiser"; new, no reference counterpart)
TEMPORAL_DTYPE = np.dtype([("worldPosition", "<f4", 3), ("hitDistance", "<f4"), ("worldNormal", "<f4", 3), ("filterable", "<f4"),
                           ("colour", "<f4", 3), ("N", "<f4"), ("m1", "<f4"), ("m2", "<f4"), ("variance", "<f4"), ("pad", "<f4")])
assert TEMPORAL_DTYPE.itemsize == 64
# the upscaler's hi-res guide record (include/fyprt.h, "upscaler"; new, no reference counterpart)
UPSCALE_GUIDE_DTYPE = np.dtype([("worldPosition", "<f4", 3), ("hitDistance", "<f4"), ("worldNormal", "<f4", 3), ("filterable", "<f4")])
assert UPSCALE_GUIDE_DTYPE.itemsize == 32
BUFFER_DTYPES = {BUF_ACCUM: np.dtype(("<f4", 4)), BUF_IMAGE: np.dtype("<u4"), BUF_PAYLOAD: PAYLOAD_DTYPE,
                 BUF_DEPTH: np.dtype("<f4"), BUF_NORMAL: np.dtype(("<f4", 2)), BUF_DI: DI_DTYPE, BUF_DI_PREV: DI_DTYPE,
                 BUF_GI: GI_DTYPE, BUF_GI_PREV: GI_DTYPE, BUF_ALBEDO: np.dtype(("<f4", 4)), BUF_TEMPORAL: TEMPORAL_DTYPE,
                 BUF_UPSCALE_GUIDE: UPSCALE_GUIDE_DTYPE, BUF_UPSCALE_ALBEDO: np.dtype(("<f4", 4))}

VERTEX_DTYPE = np.dtype([("position", "<f4", 3), ("normal", "<f4", 3), ("uv", "<f4", 2)])
TRIANGLE_DTYPE = np.dtype([("v0", "<u4"), ("v1", "<u4"), ("v2", "<u4"), ("materialIndex", "<i4")])
MATERIAL_DTYPE = np.dtype([("isUseAlbedoMap", "<u4"), ("albedo", "<f4", 3), ("albedoMapIndex", "<u4"),
                           ("roughness", "<f4"), ("metallic", "<f4"), ("emissionColor", "<f4", 3),
                           ("emissionPower", "<f4")])
MESH_DTYPE = np.dtype([("firstTriangle", "<u4"), ("triangleCount", "<u4"), ("materialIndex", "<i4")])
LT_NODE_DTYPE = np.dtype([("energy", "<f4"), ("numEmitters", "<u4"), ("left", "<u4"), ("rightOrEmitter", "<u4"),
                          ("isLeaf", "<u4"), ("coneAxis", "<f4", 3), ("theta_o", "<f4"), ("theta_e", "<f4"),
                          ("boxLo", "<f4", 3), ("boxHi", "<f4", 3), ("boxCentroid", "<f4", 3), ("_pad", "<u4")])
assert VERTEX_DTYPE.itemsize == 32 and TRIANGLE_DTYPE.itemsize == 16 and MATERIAL_DTYPE.itemsize == 44
assert MESH_DTYPE.itemsize == 12 and LT_NODE_DTYPE.itemsize == 80
# batched ray queries (fyprt_trace_rays): fyprt_ray (32 B) and the two query kinds
RAY_DTYPE = np.dtype([("origin", "<f4", 3), ("tmin", "<f4"), ("direction", "<f4", 3), ("tmax", "<f4")])
assert RAY_DTYPE.itemsize == 32
QUERY_CLOSEST, QUERY_OCCLUDED = 0, 1
# multi-hit queries (fyprt_trace_ray_hits): fyprt_ray_hit (16 B); the unused record is (-1, 0xFFFFFFFF, 0, 0)
RAY_HIT_DTYPE = np.dtype([("t", "<f4"), ("triangle", "<u4"), ("u", "<f4"), ("v", "<f4")])
assert RAY_HIT_DTYPE.itemsize == 16
QUERY_MAX_HITS = 8               # FYPRT_QUERY_MAX_HITS
# nearest-point queries (fyprt_nearest_points): fyprt_point and fyprt_point_hit (16 B each); the unused record as above
POINT_DTYPE = np.dtype([("position", "<f4", (3,)), ("max_distance", "<f4")])
POINT_HIT_DTYPE = np.dtype([("distance2", "<f4"), ("triangle", "<u4"), ("u", "<f4"), ("v", "<f4")])
assert POINT_DTYPE.itemsize == 16 and POINT_HIT_DTYPE.itemsize == 16
# box-overlap queries (fyprt_overlap_boxes): fyprt_box (32 B; the pads are ignored); the answers are bare uint32 triangle indices
BOX_DTYPE = np.dtype([("lo", "<f4", (3,)), ("pad0", "<u4"), ("hi", "<f4", (3,)), ("pad1", "<u4")])
assert BOX_DTYPE.itemsize == 32
OVERLAP_MAX_HITS = 32            # FYPRT_OVERLAP_MAX_HITS
# triangle-overlap queries (fyprt_overlap_triangles): fyprt_triangle (48 B; the pads are ignored); answers as the box query's
# (TRIANGLE_DTYPE is the scene's index triangle above)
QUERY_TRIANGLE_DTYPE = np.dtype([("v0", "<f4", (3,)), ("pad0", "<u4"), ("v1", "<f4", (3,)), ("pad1", "<u4"), ("v2", "<f4", (3,)), ("pad2", "<u4")])
assert QUERY_TRIANGLE_DTYPE.itemsize == 48
NO_TRIANGLE = 0xFFFFFFFF         # an unused slot of a box's answer; as `after`, a finished box
RENDER_RAYS_CHUNK = 1 << 21      # FYPRT_RENDER_RAYS_CHUNK: rays per internal pass of fyprt_render_rays*
BVH_NODE_DTYPE = np.dtype([("origin", "<f4", 3), ("ex", "u1", 3), ("meta", "u1"), ("child", "<i4", 4),
                           ("qlo", "u1", (3, 4)), ("qhi", "u1", (3, 4)), ("pad", "<u4", 2)])
BVH_TRI_DTYPE = np.dtype([("v0", "<f4", 3), ("e1", "<f4", 3), ("e2", "<f4", 3), ("tri", "<u4"), ("pad", "<u4", 2)])
assert BVH_NODE_DTYPE.itemsize == 64 and BVH_TRI_DTYPE.itemsize == 48


class Settings(C.Structure):  # RenderingSettings.h:5-22 (52 B) with the reference's defaults
    _fields_ = [("to_accumulate", C.c_uint8), ("_pad0", C.c_uint8 * 3), ("light_bounces", C.c_int32),
                ("sample_count", C.c_int32), ("sky_color", C.c_float * 3), ("technique", C.c_int32),
                ("light_candidate_count", C.c_int32), ("rand_seed", C.c_uint32), ("use_temporal_reuse", C.c_uint8),
                ("use_spatial_reuse", C.c_uint8), ("_pad1", C.c_uint8 * 2), ("temporal_history_limit", C.c_int32),
                ("spatial_neighbor_num", C.c_int32), ("spatial_neighbor_radius", C.c_int32)]

    def __init__(self, **kw):
        super().__init__()
        self.to_accumulate = 1
        self.light_bounces = 1
        self.sample_count = 1
        self.sky_color = (C.c_float * 3)(1.0, 1.0, 1.0)
        self.technique = BRUTE_FORCE
        self.light_candidate_count = 4
        self.rand_seed = 1
        self.use_temporal_reuse = 0
        self.use_spatial_reuse = 0
        self.temporal_history_limit = 2
        self.spatial_neighbor_num = 5
        self.spatial_neighbor_radius = 30
        for k, v in kw.items():
            if k == "sky_color":
                self.sky_color = (C.c_float * 3)(*v)
            else:
                if not hasattr(self, k):
                    raise AttributeError(k)
                setattr(self, k, v)


assert C.sizeof(Settings) == 52


class Texture(C.Structure):
    _fields_ = [("pixels", C.c_void_p), ("width", C.c_uint32), ("height", C.c_uint32)]


class LightTrees(C.Structure):
    _fields_ = [("tlas_nodes", C.c_void_p), ("tlas_node_count", C.c_uint32), ("tlas_root", C.c_uint32),
                ("blas_nodes", C.c_void_p), ("blas_first", C.c_void_p), ("blas_count", C.c_void_p),
                ("blas_root", C.c_void_p)]


class SceneDesc(C.Structure):
    _fields_ = [("vertices", C.c_void_p), ("vertex_count", C.c_uint32),
                ("triangles", C.c_void_p), ("triangle_count", C.c_uint32), ("triangle_stride", C.c_uint32),
                ("materials", C.c_void_p), ("material_count", C.c_uint32),
                ("meshes", C.c_void_p), ("mesh_count", C.c_uint32),
                ("textures", C.POINTER(Texture)), ("texture_count", C.c_uint32),
                ("emissive_triangles", C.c_void_p), ("emissive_count", C.c_uint32),
                ("light_trees", C.POINTER(LightTrees))]


class CameraDesc(C.Structure):
    _fields_ = [("projection", C.c_float * 16), ("view", C.c_float * 16), ("prev_projection", C.c_float * 16),
                ("prev_view", C.c_float * 16), ("inverse_projection", C.c_float * 16), ("inverse_view", C.c_float * 16),
                ("position", C.c_float * 3), ("viewport_width", C.c_uint32), ("viewport_height", C.c_uint32)]


class FrameStats(C.Structure):
    _fields_ = [("kernel_ms", C.c_float), ("kernel_ms_part", C.c_float * 4), ("rays", C.c_uint64),
                ("box_tests", C.c_uint64), ("tri_tests", C.c_uint64), ("hits", C.c_uint64), ("part_rays", C.c_uint64 * 4),
                ("part_box_tests", C.c_uint64 * 4), ("part_tri_tests", C.c_uint64 * 4), ("part_hits", C.c_uint64 * 4),
                ("launches", C.c_uint32), ("node_visits", C.c_uint64), ("part_node_visits", C.c_uint64 * 4)]


class EditStats(C.Structure):  # fyprt_edit_stats: what the last geometry edit covered (fyprt_last_edit_stats)
    _fields_ = [("partial", C.c_uint32), ("triangles_refreshed", C.c_uint32), ("leaf_records_refreshed", C.c_uint32),
                ("nodes_refit", C.c_uint32), ("level_launches", C.c_uint32)]


class AppendPlacement(C.Structure):  # fyprt_append_placement: where the last append linked its sub-tree (fyprt_last_append_placement)
    _fields_ = [("mode", C.c_uint32), ("kind", C.c_uint32), ("node", C.c_uint32), ("slot", C.c_uint32), ("depth", C.c_uint32),
                ("cost_bits", C.c_uint32), ("levels_before", C.c_uint32), ("levels_after", C.c_uint32), ("candidates", C.c_uint32)]


class TreeCost(C.Structure):  # fyprt_tree_cost_sums (40 B): the surface-area cost of the tree as it is (fyprt_tree_cost)
    _fields_ = [("root_area", C.c_double), ("inner_area", C.c_double), ("leaf_area", C.c_double),
                ("nodes", C.c_uint32), ("leaf_children", C.c_uint32), ("leaf_records", C.c_uint32), ("levels", C.c_uint32)]


assert C.sizeof(TreeCost) == 40


class DenoiseParams(C.Structure):  # fyprt_denoise_params (20 B) with the library's defaults (fyprt_denoise_default_params)
    _fields_ = [("iterations", C.c_uint32), ("sigma_luminance", C.c_float), ("sigma_plane", C.c_float),
                ("normal_power_log2", C.c_uint32), ("demodulate_albedo", C.c_uint32)]

    def __init__(self, **kw):
        super().__init__()
        self.iterations, self.sigma_luminance, self.sigma_plane, self.normal_power_log2, self.demodulate_albedo = 5, 4.0, 0.01, 6, 1
        for k, v in kw.items():
            if not hasattr(self, k):
                raise AttributeError(k)
            setattr(self, k, v)


assert C.sizeof(DenoiseParams) == 20


class TemporalParams(C.Structure):  # fyprt_temporal_params (36 B) with the library's defaults (fyprt_denoise_temporal_default_params)
    _fields_ = [("spatial", DenoiseParams), ("history_limit", C.c_uint32), ("normal_min", C.c_float), ("plane_max", C.c_float),
                ("feedback", C.c_uint32)]

    def __init__(self, **kw):
        """Keywords: the four fields of this struct, `spatial` (a DenoiseParams), or any field of DenoiseParams (set on `spatial`)."""
        super().__init__()
        self.spatial = DenoiseParams()
        self.history_limit, self.normal_min, self.plane_max, self.feedback = 32, 0.9, 0.02, 1
        for k, v in kw.items():
            if hasattr(self, k):
                setattr(self, k, v)
            elif hasattr(self.spatial, k):
                setattr(self.spatial, k, v)
            else:
                raise AttributeError(k)


assert C.sizeof(TemporalParams) == 36


class UpscaleParams(C.Structure):  # fyprt_upscale_params (44 B) with the library's defaults (fyprt_upscale_default_params)
    _fields_ = [("scale", C.c_uint32), ("temporal", C.c_uint32), ("filter", TemporalParams)]

    def __init__(self, **kw):
        """Keywords: `scale`, `temporal`, `filter` (a TemporalParams), or any keyword of TemporalParams (set on `filter`)."""
        super().__init__()
        self.scale, self.temporal = 2, 0
        self.filter = TemporalParams()
        for k, v in kw.items():
            if hasattr(self, k):
                setattr(self, k, v)
            elif hasattr(self.filter, k):
                setattr(self.filter, k, v)
            elif hasattr(self.filter.spatial, k):
                setattr(self.filter.spatial, k, v)
            else:
                raise AttributeError(k)


assert C.sizeof(UpscaleParams) == 44


EXPORTED_SYMBOLS = [
    "fyprt_create", "fyprt_destroy", "fyprt_last_error", "fyprt_resize", "fyprt_set_rows", "fyprt_upload_scene",
    "fyprt_set_camera", "fyprt_render", "fyprt_render_async", "fyprt_synchronize", "fyprt_readback",
    "fyprt_image_device_ptr", "fyprt_set_external_image", "fyprt_stream", "fyprt_read_buffer", "fyprt_frame_timings",
    "fyprt_reset_frame_index", "fyprt_frame_index", "fyprt_export_bvh", "fyprt_export_lighttrees", "fyprt_get_tuning", "fyprt_update_vertices",
    "fyprt_set_ray_counting", "fyprt_set_tuning", "fyprt_version",
    "fyprt_group_create", "fyprt_group_destroy", "fyprt_group_set_rows", "fyprt_group_set_halo_mode", "fyprt_group_render", "fyprt_group_gather",
    "fyprt_group_synchronize", "fyprt_comm_unique_id", "fyprt_comm_init_rank", "fyprt_comm_set_rows", "fyprt_comm_set_halo_mode", "fyprt_comm_render",
    "fyprt_comm_gather", "fyprt_comm_destroy", "fyprt_render_part", "fyprt_balance_rows", "fyprt_last_frame_ms", "fyprt_halo_plan", "fyprt_comm_ops",
    "fyprt_set_object_vertices", "fyprt_update_transforms", "fyprt_compare_image",
    "fyprt_set_row_stripes", "fyprt_group_set_interleave", "fyprt_comm_set_interleave", "fyprt_selftest_math",
    "fyprt_trace_rays", "fyprt_trace_rays_device",
    "fyprt_trace_ray_hits", "fyprt_trace_ray_hits_device",
    "fyprt_render_rays", "fyprt_render_rays_device",
    "fyprt_denoise_default_params", "fyprt_denoise", "fyprt_denoise_device",
    "fyprt_denoise_temporal_default_params", "fyprt_denoise_temporal", "fyprt_denoise_temporal_device", "fyprt_denoise_temporal_reset",
    "fyprt_live_device_bytes",
    "fyprt_update_materials", "fyprt_export_emissive",
    "fyprt_denoise_temporal_set_motion",
    "fyprt_group_denoise", "fyprt_group_denoise_device", "fyprt_group_denoise_plan",
    "fyprt_append_meshes", "fyprt_append_textures", "fyprt_remove_meshes",
    "fyprt_group_denoise_temporal", "fyprt_group_denoise_temporal_device", "fyprt_group_denoise_temporal_reset",
    "fyprt_group_denoise_temporal_plan",
    "fyprt_upscale_default_params", "fyprt_denoise_upscale", "fyprt_denoise_upscale_device",
    "fyprt_selftest_functions",
    "fyprt_group_denoise_upscale", "fyprt_group_denoise_upscale_device", "fyprt_group_denoise_upscale_plan",
    "fyprt_update_mesh_vertices", "fyprt_last_edit_stats",
    "fyprt_set_append_placement", "fyprt_last_append_placement",
    "fyprt_regraft_meshes", "fyprt_tree_cost",
    "fyprt_kept_primary_frames",
    "fyprt_nearest_points", "fyprt_nearest_points_device",
    "fyprt_overlap_boxes", "fyprt_overlap_boxes_device",
    "fyprt_overlap_triangles", "fyprt_overlap_triangles_device",
    "fyprt_set_mesh_query_masks", "fyprt_set_query_mask", "fyprt_get_query_filter",
]
# enum fyprt_probe (fyprt_selftest_functions) and the 32-bit words of one input / output record of each probe
(PROBE_SINCOS, PROBE_ACOS, PROBE_POW5, PROBE_RND, PROBE_OCT_ENCODE, PROBE_OCT_DECODE, PROBE_PACK_ABGR, PROBE_UNPACK_ABGR, PROBE_EVAL_BRDF,
 PROBE_PDF_BRDF, PROBE_PDF_GGX, PROBE_SAMPLE_UNIFORM, PROBE_SAMPLE_COSINE, PROBE_SAMPLE_GGX, PROBE_SAMPLE_BRDF, PROBE_DI_UPDATE,
 PROBE_SAMPLE_ALBEDO, PROBE_CLUSTER_IMPORTANCE, PROBE_CLUSTER_IMPORTANCE_GENERAL, PROBE_ASIN_KERNEL) = range(20)
PROBE_IN_WORDS = (1, 1, 1, 1, 3, 2, 4, 1, 16, 16, 16, 16, 16, 16, 16, 4, 3, 23, 23, 2)
PROBE_OUT_WORDS = (2, 1, 1, 2, 2, 3, 1, 4, 3, 1, 1, 5, 5, 5, 5, 7, 3, 1, 1, 2)
GROUP_HISTORY_ROWS = 32   # FYPRT_GROUP_HISTORY_ROWS: the default history window of Group.denoise_temporal, rows either side of a band


class FyprtError(RuntimeError):
    pass


_lib = None


def load_library(path: os.PathLike | None = None) -> C.CDLL:
    """Load libfyprt.so (built by __graft_entry__.build() / csrc/build.sh). Fails loudly."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = Path(path) if path else Path(os.environ.get("FYPRT_LIB", LIB_PATH))     # FYPRT_LIB: an alternative build (A/B experiments)
    if not p.exists():
        raise FyprtError(f"HIP extension not built: {p} is missing. Run `python __graft_entry__.py build` "
                         f"(hipcc --offload-arch=gfx950). There is no CPU fallback for the product path.")
    lib = C.CDLL(str(p))
    vp, u32, i32 = C.c_void_p, C.c_uint32, C.c_int32
    lib.fyprt_create.argtypes = [C.c_int, C.POINTER(vp)]
    lib.fyprt_destroy.argtypes = [vp]
    lib.fyprt_destroy.restype = None
    lib.fyprt_last_error.argtypes = [vp]
    lib.fyprt_last_error.restype = C.c_char_p
    lib.fyprt_resize.argtypes = [vp, u32, u32]
    lib.fyprt_set_rows.argtypes = [vp, u32, u32, u32]
    lib.fyprt_upload_scene.argtypes = [vp, C.POINTER(SceneDesc)]
    lib.fyprt_set_camera.argtypes = [vp, C.POINTER(CameraDesc)]
    lib.fyprt_render.argtypes = [vp, C.POINTER(Settings), C.POINTER(FrameStats)]
    lib.fyprt_render_async.argtypes = [vp, C.POINTER(Settings)]
    lib.fyprt_synchronize.argtypes = [vp]
    lib.fyprt_frame_timings.argtypes = [vp, u32, C.POINTER(C.c_float * 4), C.POINTER(u32)]
    lib.fyprt_readback.argtypes = [vp, vp, vp]
    lib.fyprt_image_device_ptr.argtypes = [vp, C.POINTER(vp)]
    lib.fyprt_set_external_image.argtypes = [vp, vp]
    lib.fyprt_stream.argtypes = [vp, C.POINTER(vp)]
    lib.fyprt_read_buffer.argtypes = [vp, C.c_int, vp, C.c_size_t]
    lib.fyprt_reset_frame_index.argtypes = [vp]
    lib.fyprt_frame_index.argtypes = [vp]
    lib.fyprt_frame_index.restype = u32
    lib.fyprt_update_vertices.argtypes = [vp, vp, u32]
    lib.fyprt_get_tuning.argtypes = [vp, C.c_int, C.POINTER(C.c_int)]
    lib.fyprt_export_bvh.argtypes = [vp, vp, C.POINTER(u32), vp, C.POINTER(u32), C.POINTER(i32), C.POINTER(u32)]
    lib.fyprt_export_lighttrees.argtypes = [vp, vp, C.POINTER(u32), C.POINTER(u32), vp, C.POINTER(u32), vp, vp, vp]
    lib.fyprt_set_ray_counting.argtypes = [vp, C.c_int]
    lib.fyprt_set_tuning.argtypes = [vp, C.c_int, C.c_int]
    lib.fyprt_version.restype = C.c_char_p
    if hasattr(lib, "fyprt_live_device_bytes"):   # (absent only in older builds loaded through FYPRT_LIB for an A/B run)
        lib.fyprt_live_device_bytes.argtypes = []
        lib.fyprt_live_device_bytes.restype = C.c_uint64
    lib.fyprt_set_object_vertices.argtypes = [vp, vp, u32, C.POINTER(u32)]
    lib.fyprt_update_transforms.argtypes = [vp, C.POINTER(u32), C.POINTER(C.c_float), u32]
    lib.fyprt_update_mesh_vertices.argtypes = [vp, C.POINTER(u32), u32, vp, u32]
    lib.fyprt_last_edit_stats.argtypes = [vp, C.POINTER(EditStats)]
    if hasattr(lib, "fyprt_set_append_placement"):  # (absent only in older builds loaded through FYPRT_LIB for an A/B run)
        lib.fyprt_set_append_placement.argtypes = [vp, C.c_int]
        lib.fyprt_last_append_placement.argtypes = [vp, C.POINTER(AppendPlacement)]
    if hasattr(lib, "fyprt_kept_primary_frames"):   # (absent only in older builds loaded through FYPRT_LIB for an A/B run)
        lib.fyprt_kept_primary_frames.argtypes = [vp, C.POINTER(C.c_uint64)]
    lib.fyprt_compare_image.argtypes = [vp, vp, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double)]
    if hasattr(lib, "fyprt_update_materials"):   # (absent only in older builds loaded through FYPRT_LIB for an A/B run)
        lib.fyprt_update_materials.argtypes = [vp, vp, u32, C.POINTER(u32), C.POINTER(i32), u32, vp, u32]
        lib.fyprt_export_emissive.argtypes = [vp, vp, C.POINTER(u32)]
    if hasattr(lib, "fyprt_trace_rays"):     # (absent only in older builds loaded through FYPRT_LIB for an A/B run)
        lib.fyprt_trace_rays.argtypes = [vp, C.c_int, vp, u32, vp, C.POINTER(FrameStats)]
        lib.fyprt_trace_rays_device.argtypes = [vp, C.c_int, vp, u32, vp]
    if hasattr(lib, "fyprt_trace_ray_hits"):
        lib.fyprt_trace_ray_hits.argtypes = [vp, vp, vp, u32, u32, vp, vp, C.POINTER(FrameStats)]
        lib.fyprt_trace_ray_hits_device.argtypes = [vp, vp, vp, u32, u32, vp, vp]
    if hasattr(lib, "fyprt_nearest_points"):   # (absent only in older builds loaded through FYPRT_LIB for an A/B run)
        lib.fyprt_nearest_points.argtypes = [vp, vp, vp, u32, u32, vp, vp, C.POINTER(FrameStats)]
        lib.fyprt_nearest_points_device.argtypes = [vp, vp, vp, u32, u32, vp, vp]
    if hasattr(lib, "fyprt_overlap_boxes"):
        lib.fyprt_overlap_boxes.argtypes = [vp, vp, vp, u32, u32, vp, vp, vp, C.POINTER(FrameStats)]
        lib.fyprt_overlap_boxes_device.argtypes = [vp, vp, vp, u32, u32, vp, vp, vp]
    if hasattr(lib, "fyprt_overlap_triangles"):
        lib.fyprt_overlap_triangles.argtypes = [vp, vp, vp, u32, u32, vp, vp, vp, C.POINTER(FrameStats)]
        lib.fyprt_overlap_triangles_device.argtypes = [vp, vp, vp, u32, u32, vp, vp, vp]
    if hasattr(lib, "fyprt_set_mesh_query_masks"):
        lib.fyprt_set_mesh_query_masks.argtypes = [vp, vp, u32]
        lib.fyprt_set_query_mask.argtypes = [vp, u32]
        lib.fyprt_get_query_filter.argtypes = [vp, vp, C.POINTER(u32), C.POINTER(u32), C.POINTER(C.c_uint64)]
    if hasattr(lib, "fyprt_render_rays"):    # (absent only in older builds loaded through FYPRT_LIB for an A/B run)
        lib.fyprt_render_rays.argtypes = [vp, C.POINTER(Settings), u32, vp, vp, u32, u32, vp, vp, C.POINTER(FrameStats)]
        lib.fyprt_render_rays_device.argtypes = [vp, C.POINTER(Settings), u32, vp, vp, u32, u32, vp, vp]
    if hasattr(lib, "fyprt_denoise"):        # (absent only in older builds loaded through FYPRT_LIB for an A/B run)
        lib.fyprt_denoise_default_params.argtypes = [C.POINTER(DenoiseParams)]
        lib.fyprt_denoise.argtypes = [vp, C.POINTER(DenoiseParams), vp, vp, C.POINTER(FrameStats)]
        lib.fyprt_denoise_device.argtypes = [vp, C.POINTER(DenoiseParams), vp, vp]
    if hasattr(lib, "fyprt_denoise_temporal"):   # (absent only in older builds loaded through FYPRT_LIB for an A/B run)
        lib.fyprt_denoise_temporal_default_params.argtypes = [C.POINTER(TemporalParams)]
        lib.fyprt_denoise_temporal.argtypes = [vp, C.POINTER(TemporalParams), vp, vp, C.POINTER(FrameStats)]
        lib.fyprt_denoise_temporal_device.argtypes = [vp, C.POINTER(TemporalParams), vp, vp]
        lib.fyprt_denoise_temporal_reset.argtypes = [vp]
    if hasattr(lib, "fyprt_denoise_upscale"):    # (absent only in older builds loaded through FYPRT_LIB for an A/B run)
        lib.fyprt_upscale_default_params.argtypes = [C.POINTER(UpscaleParams)]
        lib.fyprt_denoise_upscale.argtypes = [vp, C.POINTER(UpscaleParams), vp, vp, C.POINTER(FrameStats)]
        lib.fyprt_denoise_upscale_device.argtypes = [vp, C.POINTER(UpscaleParams), vp, vp]
    if hasattr(lib, "fyprt_denoise_temporal_set_motion"):   # (absent only in older builds loaded through FYPRT_LIB for an A/B run)
        lib.fyprt_denoise_temporal_set_motion.argtypes = [vp, C.c_int]
    lib.fyprt_group_create.argtypes = [C.POINTER(vp), C.c_int, C.POINTER(u32), C.POINTER(vp)]
    lib.fyprt_group_destroy.argtypes = [vp]
    lib.fyprt_group_destroy.restype = None
    lib.fyprt_group_set_rows.argtypes = [vp, C.POINTER(u32)]
    lib.fyprt_group_set_halo_mode.argtypes = [vp, C.c_int]
    lib.fyprt_group_set_interleave.argtypes = [vp, u32]
    lib.fyprt_comm_set_interleave.argtypes = [vp, u32]
    lib.fyprt_set_row_stripes.argtypes = [vp, u32, u32, u32]
    lib.fyprt_selftest_math.argtypes = [vp, C.POINTER(C.c_uint64), C.POINTER(u32)]
    if hasattr(lib, "fyprt_selftest_functions"):   # (absent only in older builds loaded through FYPRT_LIB for an A/B run)
        lib.fyprt_selftest_functions.argtypes = [vp, C.c_int, vp, u32, vp]
    lib.fyprt_group_render.argtypes = [vp, C.POINTER(Settings)]
    lib.fyprt_group_gather.argtypes = [vp, C.c_int]
    lib.fyprt_group_synchronize.argtypes = [vp]
    lib.fyprt_comm_unique_id.argtypes = [vp]
    lib.fyprt_comm_init_rank.argtypes = [vp, C.c_int, C.c_int, vp, C.POINTER(u32)]
    lib.fyprt_comm_set_rows.argtypes = [vp, C.POINTER(u32)]
    lib.fyprt_comm_set_halo_mode.argtypes = [vp, C.c_int]
    lib.fyprt_comm_render.argtypes = [vp, C.POINTER(Settings)]
    lib.fyprt_comm_gather.argtypes = [vp, C.c_int]
    lib.fyprt_comm_destroy.argtypes = [vp]
    lib.fyprt_comm_destroy.restype = None
    lib.fyprt_render_part.argtypes = [vp, C.POINTER(Settings), C.c_int]
    lib.fyprt_balance_rows.argtypes = [C.POINTER(u32), C.POINTER(C.c_float), C.c_int, u32, u32, C.POINTER(u32)]
    lib.fyprt_last_frame_ms.argtypes = [vp, C.POINTER(C.c_float)]
    lib.fyprt_halo_plan.argtypes = [C.POINTER(u32), C.c_int, u32, u32, C.c_int, C.POINTER(u32), C.c_int]
    if hasattr(lib, "fyprt_comm_ops"):       # (absent only in older builds loaded through FYPRT_LIB for an A/B run)
        lib.fyprt_comm_ops.argtypes = [C.c_int, C.POINTER(u32), C.POINTER(u32), C.c_int, u32, u32, C.c_int, u32, C.c_int, C.POINTER(u32), C.c_int, C.POINTER(C.c_uint64), C.c_int]
    if hasattr(lib, "fyprt_group_denoise"):  # (absent only in older builds loaded through FYPRT_LIB for an A/B run)
        lib.fyprt_group_denoise.argtypes = [vp, C.POINTER(DenoiseParams), vp, vp, vp]
        lib.fyprt_group_denoise_device.argtypes = [vp, C.POINTER(DenoiseParams), C.c_int, vp, vp]
        lib.fyprt_group_denoise_plan.argtypes = [C.POINTER(u32), C.c_int, u32, u32, C.POINTER(u32), C.c_int]
    if hasattr(lib, "fyprt_group_denoise_temporal"):  # (absent only in older builds loaded through FYPRT_LIB for an A/B run)
        lib.fyprt_group_denoise_temporal.argtypes = [vp, C.POINTER(TemporalParams), u32, vp, vp, vp]
        lib.fyprt_group_denoise_temporal_device.argtypes = [vp, C.POINTER(TemporalParams), u32, C.c_int, vp, vp]
        lib.fyprt_group_denoise_temporal_reset.argtypes = [vp]
        lib.fyprt_group_denoise_temporal_plan.argtypes = [C.POINTER(u32), C.c_int, u32, u32, u32, C.POINTER(u32), C.c_int]
    if hasattr(lib, "fyprt_group_denoise_upscale"):  # (absent only in older builds loaded through FYPRT_LIB for an A/B run)
        lib.fyprt_group_denoise_upscale.argtypes = [vp, C.POINTER(UpscaleParams), u32, vp, vp, vp]
        lib.fyprt_group_denoise_upscale_device.argtypes = [vp, C.POINTER(UpscaleParams), u32, C.c_int, vp, vp]
        lib.fyprt_group_denoise_upscale_plan.argtypes = [C.POINTER(u32), C.c_int, u32, u32, u32, u32, C.POINTER(u32), C.c_int]
    if hasattr(lib, "fyprt_append_meshes"):  # (absent only in older builds loaded through FYPRT_LIB for an A/B run)
        lib.fyprt_append_meshes.argtypes = [vp, vp, u32, vp, u32, u32, vp, u32, vp, C.POINTER(u32)]
        lib.fyprt_append_textures.argtypes = [vp, C.POINTER(Texture), u32]
    if hasattr(lib, "fyprt_remove_meshes"):  # (absent only in older builds loaded through FYPRT_LIB for an A/B run)
        lib.fyprt_remove_meshes.argtypes = [vp, C.POINTER(u32), u32, C.POINTER(u32)]
    if hasattr(lib, "fyprt_regraft_meshes"):  # (absent only in older builds loaded through FYPRT_LIB for an A/B run)
        lib.fyprt_regraft_meshes.argtypes = [vp, C.POINTER(u32), u32, C.POINTER(AppendPlacement)]
        lib.fyprt_tree_cost.argtypes = [vp, C.POINTER(TreeCost)]
    alternative = path is not None or "FYPRT_LIB" in os.environ      # an older build loaded for an A/B run may lack the newest entry points
    for f in EXPORTED_SYMBOLS:
        if alternative and not hasattr(lib, f):
            continue
        getattr(lib, f)                                                # the product library must export every symbol of include/fyprt.h
    if path is None:
        _lib = lib
    return lib


def _ptr(a: np.ndarray | None):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def make_scene_desc(scene, light_trees: dict | None = None):
    """Build a fyprt_scene_desc from a host `Scene` (fypraytracer_amd.scene.Scene).
    Returns (desc, keepalive) — keep `keepalive` referenced while the desc is in use."""
    keep = []
    v = np.ascontiguousarray(scene.world_vertices, dtype=VERTEX_DTYPE)
    t = np.ascontiguousarray(scene.triangles, dtype=TRIANGLE_DTYPE)
    m = np.ascontiguousarray(scene.materials_array(), dtype=MATERIAL_DTYPE)
    ms = np.ascontiguousarray(scene.meshes_array(), dtype=MESH_DTYPE)
    keep += [v, t, m, ms]
    d = SceneDesc()
    d.vertices, d.vertex_count = _ptr(v), len(v)
    d.triangles, d.triangle_count, d.triangle_stride = _ptr(t), len(t), TRIANGLE_DTYPE.itemsize
    d.materials, d.material_count = _ptr(m), len(m)
    d.meshes, d.mesh_count = _ptr(ms), len(ms)
    texs = (Texture * max(1, len(scene.textures)))()
    for i, px in enumerate(scene.textures):
        px = np.ascontiguousarray(px, dtype=np.uint32)
        keep.append(px)
        texs[i].pixels, texs[i].height, texs[i].width = _ptr(px), px.shape[0], px.shape[1]
    keep.append(texs)
    d.textures = C.cast(texs, C.POINTER(Texture))
    d.texture_count = len(scene.textures)
    d.emissive_triangles, d.emissive_count = None, 0
    if light_trees is not None:
        lt = LightTrees()
        arrs = {k: np.ascontiguousarray(light_trees[k]) for k in ("tlas", "blas", "blas_first", "blas_count", "blas_root")}
        keep.append(arrs)
        lt.tlas_nodes, lt.tlas_node_count, lt.tlas_root = _ptr(arrs["tlas"]), len(arrs["tlas"]), int(light_trees["tlas_root"])
        lt.blas_nodes, lt.blas_first = _ptr(arrs["blas"]), _ptr(arrs["blas_first"])
        lt.blas_count, lt.blas_root = _ptr(arrs["blas_count"]), _ptr(arrs["blas_root"])
        keep.append(lt)
        d.light_trees = C.pointer(lt)
    return d, keep


def make_camera_desc(cam) -> CameraDesc:
    """From fypraytracer_amd.scene.Camera (column-major float32 4x4 matrices)."""
    c = CameraDesc()
    for name, mat in (("projection", cam.projection), ("view", cam.view), ("prev_projection", cam.prev_projection),
                      ("prev_view", cam.prev_view), ("inverse_projection", cam.inverse_projection),
                      ("inverse_view", cam.inverse_view)):
        flat = np.asarray(mat, dtype=np.float32).reshape(16)   # stored column-major already (see scene.Camera)
        setattr(c, name, (C.c_float * 16)(*flat.tolist()))
    c.position = (C.c_float * 3)(*[float(x) for x in cam.position])
    c.viewport_width, c.viewport_height = int(cam.width), int(cam.height)
    return c


def _denoise_blocking(owner, ctx, fn, args, scale, want_radiance, third, want_third):
    """The blocking form of a denoiser call of `owner` (a Context or a Group: its library, handle and _check): entry `fn` with `args`,
    then host outputs of `scale` times `ctx`'s frame (None: the frame itself), then `third` — a FrameStats, always passed, or a
    band_ms array, passed when wanted.  Returns (image, radiance or None) reshaped, with `want_third` also the stats / the list of ms."""
    s = scale or 1
    h, w = ctx.height * s, ctx.width * s
    n = max(h * w, 1) if scale else h * w
    img = np.empty(n, dtype=np.uint32)
    rad = np.empty((n, 4), dtype=np.float32) if want_radiance else None
    stats = isinstance(third, FrameStats)
    owner._check(getattr(owner.lib, fn)(owner.h, *args, _ptr(img), _ptr(rad), C.byref(third) if stats else third if want_third else None))
    out = (img.reshape(h, w), rad.reshape(h, w, 4) if want_radiance else None)
    return out + (third if stats else list(third),) if want_third else out


def _denoise_tensor(owner, ctx, gpu, who, fn, args, scale, image_tensor, radiance_tensor):
    """The device form of a denoiser call of `owner`: entry `fn` with `args`, then the output tensors, which are checked against `scale`
    times the frame of `ctx` and its GPU (`gpu`: what the message calls it), on ctx's stream (Context._on_context_stream)."""
    import torch
    if image_tensor is None and radiance_tensor is None:
        raise ValueError(f"{who}: at least one output tensor is needed")
    h, w = ctx.height * scale, ctx.width * scale
    for t, dt, shape, name in ((image_tensor, torch.int32, (h, w), "image_tensor"), (radiance_tensor, torch.float32, (h, w, 4), "radiance_tensor")):
        if t is None:
            continue
        if t.dtype != dt or tuple(t.shape) != shape or not t.is_contiguous():
            raise ValueError(f"{who}: {name} must be a contiguous {dt} tensor of shape {shape}")
        if t.device.type != "cuda" or (t.device.index if t.device.index is not None else torch.cuda.current_device()) != ctx.device:
            raise ValueError(f"{who}: {name} must be on cuda:{ctx.device}, {gpu}")
    with ctx._on_context_stream((image_tensor if image_tensor is not None else radiance_tensor).device):
        owner._check(getattr(owner.lib, fn)(owner.h, *args, C.c_void_p(image_tensor.data_ptr()) if image_tensor is not None else None,
                                            C.c_void_p(radiance_tensor.data_ptr()) if radiance_tensor is not None else None))


class Context:
    """One renderer context on one GPU — the Python face of the reference's `Renderer`
    (Renderer.h:41-56): resize / upload_scene / set_camera / render / readback."""

    def __init__(self, device: int = 0, lib: C.CDLL | None = None):
        self.lib = lib or load_library()
        h = C.c_void_p()
        rc = self.lib.fyprt_create(device, C.byref(h))
        if rc != 0:
            raise FyprtError(f"fyprt_create({device}) failed: {self.lib.fyprt_last_error(None).decode()}")
        self.h = h
        self.device = device
        self.width = self.height = 0
        self._upscale = 1        # the scale of the last denoise_upscale* call: read_buffer sizes the two BUF_UPSCALE_* buffers by it
        self._keep = None

    def _check(self, rc):
        if rc != 0:
            raise FyprtError(f"fyprt error {rc}: {self.lib.fyprt_last_error(self.h).decode()}")

    def close(self):
        if getattr(self, "h", None):
            self.lib.fyprt_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def resize(self, width, height):
        self._check(self.lib.fyprt_resize(self.h, width, height))
        self.width, self.height = width, height
        self._upscale = 1

    def set_rows(self, row_begin, row_end, halo_rows=0):
        self._check(self.lib.fyprt_set_rows(self.h, row_begin, row_end, halo_rows))

    def selftest_math(self):
        """(mismatch counts, first offending argument bits) of the lean sqrt / 1/x / 1/sqrt(x) over all 2^32 arguments each."""
        n, f = (C.c_uint64 * 3)(), (C.c_uint32 * 3)()
        self._check(self.lib.fyprt_selftest_math(self.h, n, f))
        return list(n), list(f)

    def selftest_functions(self, probe, records):
        """Shading function `probe` (PROBE_*) on the device for every row of `records`, a (count, PROBE_IN_WORDS[probe]) array of
        32-bit words (uint32 or float32; include/fyprt.h lists the layouts).  Returns the (count, PROBE_OUT_WORDS[probe]) uint32 result words."""
        a = np.ascontiguousarray(records)
        if not (0 <= probe < len(PROBE_IN_WORDS)):
            self._check(self.lib.fyprt_selftest_functions(self.h, probe, None, 0, None))
        assert a.dtype.itemsize == 4 and a.ndim == 2 and a.shape[1] == PROBE_IN_WORDS[probe], (a.dtype, a.shape)
        out = np.zeros((a.shape[0], PROBE_OUT_WORDS[probe]), dtype=np.uint32)
        self._check(self.lib.fyprt_selftest_functions(self.h, probe, _ptr(a) if len(a) else None, len(a), _ptr(out) if len(a) else None))
        return out

    def set_row_stripes(self, stripe_rows, parts=1, part=0):
        """Interleaved split of the per-pixel techniques: this context renders stripes part, part + parts, ... (0 rows = off)."""
        self._check(self.lib.fyprt_set_row_stripes(self.h, stripe_rows, parts, part))

    def upload_scene(self, scene, light_trees=None):
        d, keep = make_scene_desc(scene, light_trees)
        self._check(self.lib.fyprt_upload_scene(self.h, C.byref(d)))
        self._has_object_vertices = False                         # an upload drops the object-space copy

    def set_camera(self, cam):
        c = make_camera_desc(cam)
        self._check(self.lib.fyprt_set_camera(self.h, C.byref(c)))

    def render(self, settings: Settings) -> FrameStats:
        st = FrameStats()
        self._check(self.lib.fyprt_render(self.h, C.byref(settings), C.byref(st)))
        return st

    def render_async(self, settings: Settings):
        self._check(self.lib.fyprt_render_async(self.h, C.byref(settings)))

    def render_part(self, settings: Settings, part: int):
        """One of the two parts of a ReSTIR frame (asynchronous): what a host with its own transport for the halo rows calls."""
        self._check(self.lib.fyprt_render_part(self.h, C.byref(settings), part))

    def synchronize(self):
        self._check(self.lib.fyprt_synchronize(self.h))

    def frame_timings(self, frames_back=0):
        """(per-launch ms [4], launches) of the frame enqueued `frames_back` frames ago; synchronize() first."""
        ms, n = (C.c_float * 4)(), C.c_uint32()
        self._check(self.lib.fyprt_frame_timings(self.h, frames_back, C.byref(ms), C.byref(n)))
        return list(ms), n.value

    def readback(self, want_accum=True):
        n = self.width * self.height
        img = np.empty(n, dtype=np.uint32)
        acc = np.empty((n, 4), dtype=np.float32) if want_accum else None
        self._check(self.lib.fyprt_readback(self.h, _ptr(img), _ptr(acc)))
        return img.reshape(self.height, self.width), (acc.reshape(self.height, self.width, 4) if want_accum else None)

    def read_buffer(self, which) -> np.ndarray:
        dt = BUFFER_DTYPES[which]
        s = self._upscale if which in (BUF_UPSCALE_GUIDE, BUF_UPSCALE_ALBEDO) else 1       # (flat, as every buffer: s*height rows of s*width)
        out = np.empty(self.width * s * self.height * s, dtype=dt)
        self._check(self.lib.fyprt_read_buffer(self.h, which, _ptr(out), out.nbytes))
        return out

    def image_device_ptr(self) -> int:
        p = C.c_void_p()
        self._check(self.lib.fyprt_image_device_ptr(self.h, C.byref(p)))
        return p.value

    def set_external_image(self, device_ptr: int):
        self._check(self.lib.fyprt_set_external_image(self.h, C.c_void_p(device_ptr)))

    def stream(self) -> int:
        p = C.c_void_p()
        self._check(self.lib.fyprt_stream(self.h, C.byref(p)))
        return p.value or 0

    def reset_frame_index(self):
        self._check(self.lib.fyprt_reset_frame_index(self.h))

    @property
    def frame_index(self) -> int:
        return int(self.lib.fyprt_frame_index(self.h))

    def set_ray_counting(self, on: bool):
        self._check(self.lib.fyprt_set_ray_counting(self.h, 1 if on else 0))

    def set_tuning(self, key: int, value: int):
        self._check(self.lib.fyprt_set_tuning(self.h, key, value))

    def update_vertices(self, scene):
        """Moved geometry, same topology: refit on the device (fyprt_update_vertices)."""
        v = np.ascontiguousarray(scene.world_vertices)
        self._check(self.lib.fyprt_update_vertices(self.h, v.ctypes.data, len(v)))

    def set_object_vertices(self, scene):
        """Object-space vertices + per-mesh vertex ranges (scene.mesh_transforms), for update_transforms."""
        v = np.ascontiguousarray(scene.vertices)
        first = [tr["vertex_start"] for tr in scene.mesh_transforms] + [len(v)]
        self._check(self.lib.fyprt_set_object_vertices(self.h, v.ctypes.data, len(v), (C.c_uint32 * len(first))(*first)))
        self._has_object_vertices = True                          # append_meshes passes the new meshes' object-space vertices along

    def update_transforms(self, scene, mesh_indices, matrices=None):
        """A transform edit applied on the device: 64 bytes per mesh (Scene.mesh_matrix) instead of its vertices.  `matrices`: one
        [col][row] matrix per listed mesh to apply instead of the scene's current ones (the host scene is then not read)."""
        if matrices is None:
            matrices = [scene.mesh_matrix(m) for m in mesh_indices]
        if len(matrices) != len(mesh_indices):
            raise ValueError("update_transforms: one matrix per mesh index")
        mats = np.ascontiguousarray(np.stack([np.asarray(M, dtype=np.float32).reshape(4, 4) for M in matrices]).reshape(-1))
        idx = (C.c_uint32 * len(mesh_indices))(*[int(m) for m in mesh_indices])
        self._check(self.lib.fyprt_update_transforms(self.h, idx, mats.ctypes.data_as(C.POINTER(C.c_float)), len(mesh_indices)))

    def update_mesh_vertices(self, scene, mesh_indices):
        """New world vertices of the listed meshes only (fyprt_update_mesh_vertices): their slices of scene.world_vertices, by the
        vertex ranges of scene.mesh_transforms, cross the bus; records and tree are refitted for what moved (partial refit)."""
        mesh_indices = [int(m) for m in mesh_indices]
        starts = [tr["vertex_start"] for tr in scene.mesh_transforms] + [len(scene.world_vertices)]
        parts = [scene.world_vertices[starts[m]:starts[m + 1]] for m in mesh_indices if 0 <= m < len(starts) - 1]
        v = np.ascontiguousarray(np.concatenate(parts) if parts else scene.world_vertices[:0], dtype=VERTEX_DTYPE)
        idx = (C.c_uint32 * max(1, len(mesh_indices)))(*mesh_indices)
        self._check(self.lib.fyprt_update_mesh_vertices(self.h, idx, len(mesh_indices), v.ctypes.data if len(v) else None, len(v)))

    def last_edit_stats(self) -> EditStats:
        """What the last update_vertices / update_transforms / update_mesh_vertices covered (fyprt_last_edit_stats)."""
        st = EditStats()
        self._check(self.lib.fyprt_last_edit_stats(self.h, C.byref(st)))
        return st

    def update_materials(self, scene, meshes=(), emissive_triangles=None):
        """A material edit applied on the device (fyprt_update_materials): the whole material table of `scene`, and for the listed
        meshes their current material index (all their triangles follow).  `emissive_triangles`: None = derive, as upload_scene."""
        m = np.ascontiguousarray(scene.materials_array(), dtype=MATERIAL_DTYPE)
        meshes = [int(k) for k in meshes]
        idx = (C.c_uint32 * max(1, len(meshes)))(*meshes)
        mat = (C.c_int32 * max(1, len(meshes)))(*[int(scene.meshes[k][2]) for k in meshes])
        em = None if emissive_triangles is None else np.ascontiguousarray(emissive_triangles, dtype=np.uint32)
        self._check(self.lib.fyprt_update_materials(self.h, _ptr(m) if len(m) else None, len(m), idx, mat, len(meshes),
                                                    None if em is None else (em.ctypes.data if len(em) else C.cast((C.c_uint32 * 1)(), C.c_void_p)),
                                                    0 if em is None else len(em)))

    def append_meshes(self, scene, first_new_mesh, with_object_vertices=None):
        """An import applied on the device (fyprt_append_meshes): the tails of a `scene` that add_new_mesh_to_scene extended by the
        meshes [first_new_mesh, len(scene.meshes)) — their triangles, and the vertices from the first of them on.  The object-space
        vertices go along when the context holds a copy (set_object_vertices on this wrapper); `with_object_vertices` overrides that."""
        first_new_mesh = int(first_new_mesh)
        ms = np.ascontiguousarray(scene.meshes_array()[first_new_mesh:], dtype=MESH_DTYPE)
        t0 = int(scene.meshes[first_new_mesh][0]) if first_new_mesh < len(scene.meshes) else len(scene.triangles)
        v0 = int(scene.mesh_transforms[first_new_mesh]["vertex_start"]) if first_new_mesh < len(scene.mesh_transforms) else len(scene.world_vertices)
        v = np.ascontiguousarray(scene.world_vertices[v0:], dtype=VERTEX_DTYPE)
        t = np.ascontiguousarray(scene.triangles[t0:], dtype=TRIANGLE_DTYPE)
        with_object = getattr(self, "_has_object_vertices", False) if with_object_vertices is None else bool(with_object_vertices)
        ov = first = None
        if with_object:
            ov = np.ascontiguousarray(scene.vertices[v0:], dtype=VERTEX_DTYPE)
            starts = [tr["vertex_start"] for tr in scene.mesh_transforms[first_new_mesh:]] + [len(scene.world_vertices)]
            first = (C.c_uint32 * len(starts))(*starts)
        self._check(self.lib.fyprt_append_meshes(self.h, _ptr(v) if len(v) else None, len(v), _ptr(t) if len(t) else None, len(t), TRIANGLE_DTYPE.itemsize,
                                                 _ptr(ms) if len(ms) else None, len(ms), None if ov is None else (ov.ctypes.data if len(ov) else C.cast((C.c_uint32 * 8)(), C.c_void_p)), first))
        self._has_object_vertices = with_object

    def set_append_placement(self, mode):
        """Where append_meshes links the sub-tree (fyprt_set_append_placement): 0 at the root (default), 1 at the cheapest place by
        the surface-area rule of include/fyprt.h."""
        self._check(self.lib.fyprt_set_append_placement(self.h, int(mode)))

    def last_append_placement(self) -> AppendPlacement:
        """Where the last append with triangles linked its sub-tree (fyprt_last_append_placement)."""
        pl = AppendPlacement()
        self._check(self.lib.fyprt_last_append_placement(self.h, C.byref(pl)))
        return pl

    def remove_meshes(self, removed, with_vertex_ranges=True):
        """A deletion applied on the device (fyprt_remove_meshes): `removed` is the record Scene.remove_meshes_from_scene returned
        (mesh indices and their vertex ranges before the edit).  Without `with_vertex_ranges` the library takes the meshes' own ranges
        from the object-space copy it holds, or removes no vertex when it holds none."""
        ms = [int(m) for m in removed["meshes"]]
        idx = (C.c_uint32 * max(1, len(ms)))(*ms)
        vr = None
        if with_vertex_ranges:
            vr = (C.c_uint32 * max(2, 2 * len(ms)))(*[int(x) for r in removed["vertex_ranges"] for x in r])
        self._check(self.lib.fyprt_remove_meshes(self.h, idx, len(ms), vr))

    def regraft_meshes(self, mesh_indices):
        """The listed meshes taken out of the tree and linked in again where they lie now (fyprt_regraft_meshes): nothing but the
        tree moves.  Returns one AppendPlacement per listed mesh, the report of its graft."""
        ms = [int(m) for m in mesh_indices]
        idx = (C.c_uint32 * max(1, len(ms)))(*ms)
        reports = (AppendPlacement * max(1, len(ms)))()
        self._check(self.lib.fyprt_regraft_meshes(self.h, idx, len(ms), reports))
        return [reports[k] for k in range(len(ms))]

    def tree_cost(self) -> TreeCost:
        """The surface-area cost of the tree as it is (fyprt_tree_cost); (inner_area + leaf_area) / root_area is the SAH estimate."""
        out = TreeCost()
        self._check(self.lib.fyprt_tree_cost(self.h, C.byref(out)))
        return out

    def append_textures(self, textures):
        """New textures behind the uploaded ones (fyprt_append_textures); each a uint32 [H][W] ABGR8 array."""
        px = [np.ascontiguousarray(t, dtype=np.uint32) for t in textures]
        texs = (Texture * max(1, len(px)))()
        for i, a in enumerate(px):
            texs[i].pixels, texs[i].height, texs[i].width = _ptr(a), a.shape[0], a.shape[1]
        self._check(self.lib.fyprt_append_textures(self.h, C.cast(texs, C.POINTER(Texture)) if px else None, len(px)))

    def export_emissive(self) -> np.ndarray:
        """The emissive-triangle list in effect (fyprt_export_emissive)."""
        n = C.c_uint32()
        self._check(self.lib.fyprt_export_emissive(self.h, None, C.byref(n)))
        out = np.empty(n.value, dtype=np.uint32)
        self._check(self.lib.fyprt_export_emissive(self.h, _ptr(out) if n.value else None, C.byref(n)))
        return out

    def compare_image(self, reference, flip_reference_rows=False):
        """(MSE, PSNR) of the current frame against `reference` (uint32 ABGR8, H x W), reduced on the device (MisUtils::ComputeMSE)."""
        ref = np.ascontiguousarray(reference, dtype=np.uint32)
        mse, psnr = C.c_double(), C.c_double()
        self._check(self.lib.fyprt_compare_image(self.h, ref.ctypes.data, 1 if flip_reference_rows else 0, C.byref(mse), C.byref(psnr)))
        return mse.value, psnr.value

    def kept_primary_frames(self) -> int:
        """ReSTIR DI frames since creation that reused the kept primary hits (tuning key 25; fyprt_kept_primary_frames)."""
        n = C.c_uint64()
        self._check(self.lib.fyprt_kept_primary_frames(self.h, C.byref(n)))
        return n.value

    # ---- query filters (fyprt_set_mesh_query_masks / fyprt_set_query_mask): they apply to the query methods below as they are
    def set_mesh_query_masks(self, masks):
        """One 32-bit group mask per mesh of the uploaded scene (fyprt_set_mesh_query_masks); None switches the filter off.  With a
        table set the ray, multi-hit, nearest-point and box queries see the triangles of mesh m iff masks[m] & query mask != 0."""
        if masks is None:
            self._check(self.lib.fyprt_set_mesh_query_masks(self.h, None, 0))
            return
        m = np.ascontiguousarray(masks, dtype=np.uint32).reshape(-1)
        self._check(self.lib.fyprt_set_mesh_query_masks(self.h, m.ctypes.data if len(m) else C.cast((C.c_uint32 * 1)(), C.c_void_p), len(m)))

    def set_query_mask(self, mask: int):
        """The mask of all later query calls (fyprt_set_query_mask); 0xFFFFFFFF by default."""
        self._check(self.lib.fyprt_set_query_mask(self.h, int(mask) & 0xFFFFFFFF))

    def query_filter(self):
        """(table or None when the filter is off, query mask, builds of the device data since creation) — fyprt_get_query_filter."""
        n, q, b = C.c_uint32(), C.c_uint32(), C.c_uint64()
        self._check(self.lib.fyprt_get_query_filter(self.h, None, C.byref(n), C.byref(q), C.byref(b)))
        if n.value == 0:
            return None, q.value, b.value
        out = np.empty(n.value, dtype=np.uint32)
        self._check(self.lib.fyprt_get_query_filter(self.h, out.ctypes.data, C.byref(n), C.byref(q), C.byref(b)))
        return out, q.value, b.value

    def get_tuning(self, key: int) -> int:
        v = C.c_int()
        self._check(self.lib.fyprt_get_tuning(self.h, key, C.byref(v)))
        return v.value

    def export_bvh(self):
        nn, nt, root, depth = C.c_uint32(), C.c_uint32(), C.c_int32(), C.c_uint32()
        self._check(self.lib.fyprt_export_bvh(self.h, None, C.byref(nn), None, C.byref(nt), C.byref(root), C.byref(depth)))
        nodes = np.empty(nn.value, dtype=BVH_NODE_DTYPE)
        tris = np.empty(nt.value, dtype=BVH_TRI_DTYPE)
        self._check(self.lib.fyprt_export_bvh(self.h, _ptr(nodes), C.byref(nn), _ptr(tris), C.byref(nt), C.byref(root), C.byref(depth)))
        return {"nodes": nodes, "tris": tris, "root": root.value, "max_stack": depth.value, "stack_budget": self.get_tuning(8), "skip_dead_rays": self.get_tuning(18)}

    # ---- what the query entry points share: record packing, argument checks, the torch stream hand-over, the continuation loop
    @staticmethod
    def _ray_records(who, origins, directions, tmin, tmax):
        o = np.asarray(origins, dtype=np.float32).reshape(-1, 3)
        d = np.asarray(directions, dtype=np.float32).reshape(-1, 3)
        if o.shape != d.shape:
            raise ValueError(f"{who}: {len(o)} origins but {len(d)} directions")
        n = len(o)
        rays = np.empty(n, dtype=RAY_DTYPE)
        rays["origin"], rays["direction"] = o, d
        rays["tmin"] = np.broadcast_to(np.asarray(tmin, dtype=np.float32), (n,))
        rays["tmax"] = np.broadcast_to(np.asarray(tmax, dtype=np.float32), (n,))
        return rays

    @staticmethod
    def _point_records(who, points, max_distance):
        p = np.asarray(points, dtype=np.float32)
        if p.ndim == 0 or p.size % 3 or (p.ndim > 1 and p.shape[-1] != 3):
            raise ValueError(f"{who}: points must be (N, 3), got shape {p.shape}")
        p = p.reshape(-1, 3)
        n = len(p)
        md = np.asarray(max_distance, dtype=np.float32)
        if md.ndim > 1 or (md.ndim == 1 and len(md) != n):
            raise ValueError(f"{who}: max_distance must be a scalar or {n} values")
        rec = np.empty(n, dtype=POINT_DTYPE)
        rec["position"], rec["max_distance"] = p, np.broadcast_to(md, (n,))
        return rec

    @staticmethod
    def _box_records(who, lo, hi):
        l, h = np.asarray(lo, dtype=np.float32), np.asarray(hi, dtype=np.float32)
        for name, a in (("lo", l), ("hi", h)):
            if a.ndim == 0 or a.size % 3 or (a.ndim > 1 and a.shape[-1] != 3):
                raise ValueError(f"{who}: {name} must be (N, 3), got shape {a.shape}")
        l, h = l.reshape(-1, 3), h.reshape(-1, 3)
        if len(l) != len(h):
            raise ValueError(f"{who}: {len(l)} lower but {len(h)} upper corners")
        rec = np.zeros(len(l), dtype=BOX_DTYPE)
        rec["lo"], rec["hi"] = l, h
        return rec

    @staticmethod
    def _tri_records(who, tris):
        """`tris`: (N, 3, 3) vertices, or three (N, 3) arrays (the first, second and third vertices)."""
        if isinstance(tris, (tuple, list)) and len(tris) == 3 and all(np.ndim(t) >= 1 for t in tris):
            parts = [np.asarray(t, dtype=np.float32) for t in tris]
            for name, a in zip(("v0", "v1", "v2"), parts):
                if a.size % 3 or (a.ndim > 1 and a.shape[-1] != 3) or a.ndim > 2:
                    raise ValueError(f"{who}: {name} must be (N, 3), got shape {a.shape}")
            parts = [a.reshape(-1, 3) for a in parts]
            if not len(parts[0]) == len(parts[1]) == len(parts[2]):
                raise ValueError(f"{who}: {len(parts[0])} first, {len(parts[1])} second and {len(parts[2])} third vertices")
            t = np.stack(parts, axis=1)
        else:
            t = np.asarray(tris, dtype=np.float32)
            if t.ndim not in (2, 3) or t.shape[-2:] != (3, 3):
                raise ValueError(f"{who}: tris must be (N, 3, 3) or three (N, 3) arrays, got shape {t.shape}")
            t = t.reshape(-1, 3, 3)
        rec = np.zeros(len(t), dtype=QUERY_TRIANGLE_DTYPE)
        rec["v0"], rec["v1"], rec["v2"] = t[:, 0], t[:, 1], t[:, 2]
        return rec

    @staticmethod
    def _index_after(who, after, n):
        if after is None:
            return None
        aft = np.asarray(after)
        if aft.dtype != np.uint32 or aft.size != n:
            raise ValueError(f"{who}: after must be {n} uint32 triangle indices")
        return np.ascontiguousarray(aft.reshape(-1))

    @staticmethod
    def _check_max_hits(who, max_hits, cap=QUERY_MAX_HITS):
        if not isinstance(max_hits, (int, np.integer)) or isinstance(max_hits, bool) or not 1 <= int(max_hits) <= cap:
            raise ValueError(f"{who}: max_hits must be an integer in 1..{cap}, got {max_hits!r}")
        return int(max_hits)

    @staticmethod
    def _after_records(who, after, n, dtype, dtype_name):
        if after is None:
            return None
        aft = np.asarray(after)
        if aft.dtype != dtype or aft.size != n:
            raise ValueError(f"{who}: after must be {n} {dtype_name} records")
        return np.ascontiguousarray(aft.reshape(-1))

    def _check_record_tensor(self, who, name, t, width, after=None, after_words=4):
        """`t`: the contiguous float32 (N, width) tensor of `name` on this context's GPU; `after`: None or (N, 4) beside it — for
        `after_words` 1, the box query's, an int32 (N,) tensor.  Returns N."""
        import torch
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.dim() != 2 or t.shape[1] != width or not t.is_contiguous():
            raise ValueError(f"{who}: {name} must be a contiguous float32 (N, {width}) tensor")
        if t.device.type != "cuda" or (t.device.index if t.device.index is not None else torch.cuda.current_device()) != self.device:
            raise ValueError(f"{who}: {name} must be on cuda:{self.device}, the context's GPU")
        n = t.shape[0]
        if after is not None and after_words == 1:
            if not isinstance(after, torch.Tensor) or after.dtype != torch.int32 or tuple(after.shape) != (n,) or not after.is_contiguous() or after.device != t.device:
                raise ValueError(f"{who}: after must be a contiguous int32 (N,) tensor on the {name}' device")
        elif after is not None and (after.dtype != torch.float32 or tuple(after.shape) != (n, 4) or not after.is_contiguous() or after.device != t.device):
            raise ValueError(f"{who}: after must be a contiguous float32 (N, 4) tensor on the {name}' device")
        return n

    @contextlib.contextmanager
    def _on_context_stream(self, device):
        """The ordering of every *_tensor call (trace_rays_tensor's docstring): the context stream waits for torch's current stream, the
        body enqueues on the context stream, torch's current stream waits for the context stream."""
        import torch
        cur = torch.cuda.current_stream(device)
        ext = torch.cuda.ExternalStream(self.stream(), device=device)
        ext.wait_stream(cur)                                           # inputs are written, outputs allocated before the query runs
        yield
        cur.wait_stream(ext)                                           # torch's later work (reads of the outputs, reuse of any block) follows it

    @staticmethod
    def _all_records(n, k, dtype, ask):
        """Continuation passes of a list query until every record is finished: ask(live, after) -> (hits, counts) for the records `live`
        (indices), each pass's last record per live entry passed back in as `after`.  Returns (flat records, offsets int64 (n + 1,))."""
        live = np.arange(n)                                            # records not finished yet; only they are asked again
        after = None
        parts = [[] for _ in range(n)]
        while len(live):
            hits, counts = ask(live, after)
            for j, i in enumerate(live):
                if counts[j]:
                    parts[i].append(hits[j, :counts[j]])
            go = counts == k                                           # a short list has nothing further
            live, after = live[go], np.ascontiguousarray(hits[go, k - 1])
        total = np.array([sum(len(p) for p in ps) for ps in parts], dtype=np.int64)
        offsets = np.concatenate([[0], np.cumsum(total)]).astype(np.int64)
        flat = [p for ps in parts for p in ps]
        records = np.concatenate(flat) if flat else np.empty(0, dtype=dtype)
        return records, offsets

    def trace_rays(self, origins, directions, tmin=0.0, tmax=np.inf, occluded=False, with_stats=False):
        """Batched ray query against the uploaded scene (fyprt_trace_rays, blocking).  `origins` / `directions`: (N, 3); `tmin` /
        `tmax`: scalars or (N,) arrays.  Returns the PAYLOAD_DTYPE records of the closest hits, or (occluded=True) a bool array that
        is True where any triangle lies in (tmin, tmax); with `with_stats` also the FrameStats of the launch."""
        rays = self._ray_records("trace_rays", origins, directions, tmin, tmax)
        n = len(rays)
        out = np.empty(n, dtype=np.uint32 if occluded else PAYLOAD_DTYPE)
        st = FrameStats()
        self._check(self.lib.fyprt_trace_rays(self.h, QUERY_OCCLUDED if occluded else QUERY_CLOSEST, _ptr(rays), n, _ptr(out), C.byref(st)))
        res = out.astype(bool) if occluded else out
        return (res, st) if with_stats else res

    def trace_rays_tensor(self, rays, occluded=False):
        """Batched ray query on device tensors (fyprt_trace_rays_device).  `rays`: contiguous float32 (N, 8) tensor on this context's
        GPU, one fyprt_ray per row (origin, tmin, direction, tmax).  Returns a float32 (N, 10) tensor of RayHitPayload records (column 9
        holds the int32 bits of objectIndex: `out[:, 9].view(torch.int32)`), or (occluded=True) an int32 (N,) tensor of 0 / 1.
        Ordered against torch's current stream on the device, without a host synchronisation: the context stream waits for torch's
        current stream, the query is launched, torch's current stream waits for the context stream.
        The process must have initialised torch's CUDA before the library was loaded (as bench.py does). Then the library binds to
        torch's HIP runtime and the context stream is a stream of that runtime. In the other order torch loads a second runtime and
        finds no GPU.
        No record_stream: both tensors belong to torch's current stream, and the caching allocator hands their blocks out again only to
        work on that stream, which is ordered after the query by the last wait.  record_stream would also make the allocator record an
        event on the context stream when a tensor is freed, and a tensor that outlives the context would then record on a destroyed
        stream."""
        import torch
        n = self._check_record_tensor("trace_rays_tensor", "rays", rays, 8)
        out = torch.empty((n,) if occluded else (n, 10), dtype=torch.int32 if occluded else torch.float32, device=rays.device)
        with self._on_context_stream(rays.device):
            self._check(self.lib.fyprt_trace_rays_device(self.h, QUERY_OCCLUDED if occluded else QUERY_CLOSEST, C.c_void_p(rays.data_ptr()), n,
                                                         C.c_void_p(out.data_ptr())))
        return out

    def _list_query(self, fn, rec, aft, k, hit_dtype, with_stats, totals=False):
        """One blocking list query: (hits (N, K) of `hit_dtype`, counts[, totals][, stats]); `totals`: the entry point has the box
        query's third result array."""
        n = len(rec)
        hits = np.empty((n, k), dtype=hit_dtype)
        counts = np.empty(n, dtype=np.uint32)
        extra = [np.empty(n, dtype=np.uint32)] if totals else []
        st = FrameStats()
        self._check(getattr(self.lib, fn)(self.h, _ptr(rec), _ptr(aft), n, k, _ptr(hits), _ptr(counts), *[_ptr(t) for t in extra], C.byref(st)))
        return (hits, counts, *extra, st) if with_stats else (hits, counts, *extra)

    def _list_query_tensor(self, fn, who, name, rec, width, k, after, words=4):
        """One list query on device tensors: float32 (N, K, 4) records and int32 counts; with `words` 1, the box query's, int32 (N, K)
        indices, counts and totals."""
        import torch
        n = self._check_record_tensor(who, name, rec, width, after, words)
        hits = torch.empty((n, k, 4) if words == 4 else (n, k), dtype=torch.float32 if words == 4 else torch.int32, device=rec.device)
        out = [torch.empty((n,), dtype=torch.int32, device=rec.device) for _ in range(1 if words == 4 else 2)]
        with self._on_context_stream(rec.device):
            self._check(getattr(self.lib, fn)(self.h, C.c_void_p(rec.data_ptr()), C.c_void_p(after.data_ptr()) if after is not None else None,
                                            n, k, C.c_void_p(hits.data_ptr()), *[C.c_void_p(t.data_ptr()) for t in out]))
        return (hits, *out)

    def trace_ray_hits(self, origins, directions, tmin=0.0, tmax=np.inf, max_hits=QUERY_MAX_HITS, after=None, with_stats=False):
        """Ordered multi-hit query (fyprt_trace_ray_hits, blocking): the `max_hits` nearest accepted triangles per ray, ascending by
        (t, triangle).  `origins` / `directions`: (N, 3); `tmin` / `tmax`: scalars or (N,) arrays; `after`: None or N RAY_HIT_DTYPE
        records — only hits beyond after[i] in that order are returned, and a record with t < 0 (the unused record) finishes the ray.
        Returns (hits (N, K) RAY_HIT_DTYPE, counts (N,) uint32); unused records are (-1, 0xFFFFFFFF, 0, 0); with `with_stats` also
        the FrameStats of the launch."""
        k = self._check_max_hits("trace_ray_hits", max_hits)
        rays = self._ray_records("trace_ray_hits", origins, directions, tmin, tmax)
        aft = self._after_records("trace_ray_hits", after, len(rays), RAY_HIT_DTYPE, "RAY_HIT_DTYPE")
        return self._list_query("fyprt_trace_ray_hits", rays, aft, k, RAY_HIT_DTYPE, with_stats)

    def trace_ray_hits_tensor(self, rays, max_hits, after=None):
        """Multi-hit query on device tensors (fyprt_trace_ray_hits_device).  `rays`: contiguous float32 (N, 8) tensor on this context's
        GPU, one fyprt_ray per row; `after`: None or a contiguous float32 (N, 4) tensor of hit records (the last column of records of an
        earlier call: `hits[:, -1].contiguous()`).  Returns a float32 (N, K, 4) tensor of records (t, triangle bits, u, v: the index is
        `hits[..., 1].contiguous().view(torch.int32)`) and an int32 (N,) tensor of counts.  Ordered against torch's current stream
        exactly as trace_rays_tensor is, without a host synchronisation and without record_stream."""
        k = self._check_max_hits("trace_ray_hits_tensor", max_hits)
        return self._list_query_tensor("fyprt_trace_ray_hits_device", "trace_ray_hits_tensor", "rays", rays, 8, k, after)

    def trace_all_hits(self, origins, directions, tmin=0.0, tmax=np.inf, max_hits=QUERY_MAX_HITS):
        """Every accepted hit of every ray, in order: continuation passes of trace_ray_hits (each pass's last record per ray passed
        back in as `after`) until every ray is finished.  Returns (records, offsets): flat RAY_HIT_DTYPE records, ray i's in
        records[offsets[i]:offsets[i + 1]], offsets int64 (N + 1,)."""
        k = self._check_max_hits("trace_all_hits", max_hits)
        rays = self._ray_records("trace_all_hits", origins, directions, tmin, tmax)
        return self._all_records(len(rays), k, RAY_HIT_DTYPE, lambda live, after: self.trace_ray_hits(
            rays["origin"][live], rays["direction"][live], rays["tmin"][live], rays["tmax"][live], k, after))

    def nearest_points(self, points, max_distance=np.inf, max_hits=1, after=None, with_stats=False):
        """Nearest-point query (fyprt_nearest_points, blocking): the `max_hits` closest triangles to each point, ascending by
        (distance2, triangle).  `points`: (N, 3); `max_distance`: a scalar or (N,) array, only triangles within it are answered;
        `after`: None or N POINT_HIT_DTYPE records — only triangles beyond after[i] in that order are returned, and a record with
        distance2 < 0 (the unused record) finishes the point.  Returns (hits (N, K) POINT_HIT_DTYPE, counts (N,) uint32); unused
        records are (-1, 0xFFFFFFFF, 0, 0); with `with_stats` also the FrameStats of the launch."""
        k = self._check_max_hits("nearest_points", max_hits)
        rec = self._point_records("nearest_points", points, max_distance)
        aft = self._after_records("nearest_points", after, len(rec), POINT_HIT_DTYPE, "POINT_HIT_DTYPE")
        return self._list_query("fyprt_nearest_points", rec, aft, k, POINT_HIT_DTYPE, with_stats)

    def nearest_points_tensor(self, points, max_hits, after=None):
        """Nearest-point query on device tensors (fyprt_nearest_points_device).  `points`: contiguous float32 (N, 4) tensor on this
        context's GPU, one fyprt_point per row (position, max_distance); `after`: None or a contiguous float32 (N, 4) tensor of hit
        records.  Returns a float32 (N, K, 4) tensor of records (distance2, triangle bits, u, v) and an int32 (N,) tensor of counts.
        Ordered against torch's current stream exactly as trace_rays_tensor is."""
        k = self._check_max_hits("nearest_points_tensor", max_hits)
        return self._list_query_tensor("fyprt_nearest_points_device", "nearest_points_tensor", "points", points, 4, k, after)

    def triangles_within(self, points, radius, max_hits=QUERY_MAX_HITS):
        """Every triangle within `radius` (a scalar or (N,) array) of every point, nearest first: continuation passes of nearest_points
        until every point is finished.  Returns (records, offsets) shaped as trace_all_hits': flat POINT_HIT_DTYPE records, point i's in
        records[offsets[i]:offsets[i + 1]], offsets int64 (N + 1,)."""
        k = self._check_max_hits("triangles_within", max_hits)
        rec = self._point_records("triangles_within", points, radius)
        return self._all_records(len(rec), k, POINT_HIT_DTYPE, lambda live, after: self.nearest_points(
            rec["position"][live], rec["max_distance"][live], k, after))

    def overlap_boxes(self, lo, hi, max_hits=OVERLAP_MAX_HITS, after=None, with_stats=False):
        """Box-overlap query (fyprt_overlap_boxes, blocking): the `max_hits` lowest indices of the triangles that touch each closed box
        [lo, hi].  `lo` / `hi`: (N, 3); `after`: None or N uint32 — only triangles with a greater index are returned, and NO_TRIANGLE
        (an unused slot) finishes the box.  Returns (triangles (N, K) uint32 ascending, unused slots NO_TRIANGLE; counts (N,) uint32;
        totals (N,) uint32: every accepted triangle, also those beyond K); with `with_stats` also the FrameStats of the launch."""
        k = self._check_max_hits("overlap_boxes", max_hits, OVERLAP_MAX_HITS)
        rec = self._box_records("overlap_boxes", lo, hi)
        aft = self._index_after("overlap_boxes", after, len(rec))
        return self._list_query("fyprt_overlap_boxes", rec, aft, k, np.uint32, with_stats, totals=True)

    def overlap_boxes_tensor(self, boxes, max_hits, after=None):
        """Box-overlap query on device tensors (fyprt_overlap_boxes_device).  `boxes`: contiguous float32 (N, 8) tensor on this context's
        GPU, one fyprt_box per row (lo, pad, hi, pad); `after`: None or a contiguous int32 (N,) tensor of indices (the last column of an
        earlier call: `triangles[:, -1].contiguous()`).  Returns int32 tensors: triangles (N, K) (unused slots -1), counts (N,), totals
        (N,).  Ordered against torch's current stream exactly as trace_rays_tensor is."""
        k = self._check_max_hits("overlap_boxes_tensor", max_hits, OVERLAP_MAX_HITS)
        return self._list_query_tensor("fyprt_overlap_boxes_device", "overlap_boxes_tensor", "boxes", boxes, 8, k, after, words=1)

    def triangles_in_boxes(self, lo, hi, max_hits=OVERLAP_MAX_HITS):
        """Every triangle that touches every box, ascending by index: continuation passes of overlap_boxes until every box is
        finished.  Returns (indices, offsets) shaped as triangles_within's: flat uint32 indices, box i's in
        indices[offsets[i]:offsets[i + 1]], offsets int64 (N + 1,)."""
        k = self._check_max_hits("triangles_in_boxes", max_hits, OVERLAP_MAX_HITS)
        rec = self._box_records("triangles_in_boxes", lo, hi)
        return self._all_records(len(rec), k, np.uint32, lambda live, after: self.overlap_boxes(rec["lo"][live], rec["hi"][live], k, after)[:2])

    def overlap_triangles(self, tris, max_hits=OVERLAP_MAX_HITS, after=None, with_stats=False):
        """Triangle-overlap query (fyprt_overlap_triangles, blocking): the `max_hits` lowest indices of the scene triangles that cut each
        query triangle.  `tris`: (N, 3, 3), or three (N, 3) arrays; `after`: None or N uint32 — only triangles with a greater index are
        returned, and NO_TRIANGLE (an unused slot) finishes the record.  Returns (triangles (N, K) uint32 ascending, unused slots
        NO_TRIANGLE; counts (N,) uint32; totals (N,) uint32: every accepted triangle, also those beyond K); with `with_stats` also the
        FrameStats of the launch."""
        k = self._check_max_hits("overlap_triangles", max_hits, OVERLAP_MAX_HITS)
        rec = self._tri_records("overlap_triangles", tris)
        aft = self._index_after("overlap_triangles", after, len(rec))
        return self._list_query("fyprt_overlap_triangles", rec, aft, k, np.uint32, with_stats, totals=True)

    def overlap_triangles_tensor(self, tris, max_hits, after=None):
        """Triangle-overlap query on device tensors (fyprt_overlap_triangles_device).  `tris`: contiguous float32 (N, 12) tensor on this
        context's GPU, one fyprt_triangle per row (v0, pad, v1, pad, v2, pad); `after`: None or a contiguous int32 (N,) tensor of
        indices.  Returns int32 tensors: triangles (N, K) (unused slots -1), counts (N,), totals (N,).  Ordered against torch's current
        stream exactly as trace_rays_tensor is."""
        k = self._check_max_hits("overlap_triangles_tensor", max_hits, OVERLAP_MAX_HITS)
        return self._list_query_tensor("fyprt_overlap_triangles_device", "overlap_triangles_tensor", "tris", tris, 12, k, after, words=1)

    def triangles_touching(self, tris, max_hits=OVERLAP_MAX_HITS):
        """Every scene triangle that cuts every query triangle, ascending by index: continuation passes of overlap_triangles until every
        record is finished.  Returns (indices, offsets) shaped as triangles_in_boxes'."""
        k = self._check_max_hits("triangles_touching", max_hits, OVERLAP_MAX_HITS)
        rec = self._tri_records("triangles_touching", tris)
        q = np.stack([rec["v0"], rec["v1"], rec["v2"]], axis=1)
        return self._all_records(len(rec), k, np.uint32, lambda live, after: self.overlap_triangles(q[live], k, after)[:2])

    def render_rays(self, origins, directions, settings: Settings, frame_index=1, first_index=0, pixel_indices=None, tmin=0.0, tmax=np.inf,
                    want_payload=False, with_stats=False):
        """Radiance query (fyprt_render_rays, blocking): the sample of technique `settings.technique` (0-6) for the caller's rays.
        `origins` / `directions`: (N, 3), unit directions; `tmin` / `tmax`: scalars or (N,) arrays, the primary segment's interval.
        Ray k uses the random sequence of pixel `pixel_indices[k]` (or `first_index + k`) in frame `frame_index`.  Returns float32
        (N, 4): what a frame's epilogue would add to the accumulation; with `want_payload` also the PAYLOAD_DTYPE primary records, with
        `with_stats` also the FrameStats of the call."""
        rays = self._ray_records("render_rays", origins, directions, tmin, tmax)
        n = len(rays)
        idx = None
        if pixel_indices is not None:
            idx = np.ascontiguousarray(np.asarray(pixel_indices).astype(np.uint32, copy=False).reshape(-1))
            if len(idx) != n:
                raise ValueError(f"render_rays: {n} rays but {len(idx)} pixel indices")
        rad = np.empty((n, 4), dtype=np.float32)
        pay = np.empty(n, dtype=PAYLOAD_DTYPE) if want_payload else None
        st = FrameStats()
        self._check(self.lib.fyprt_render_rays(self.h, C.byref(settings), int(frame_index), _ptr(rays), _ptr(idx), int(first_index), n,
                                               _ptr(rad), _ptr(pay), C.byref(st)))
        out = (rad,) + ((pay,) if want_payload else ()) + ((st,) if with_stats else ())
        return out[0] if len(out) == 1 else out

    def render_rays_tensor(self, rays, settings: Settings, frame_index=1, first_index=0, pixel_indices=None, want_payload=False):
        """Radiance query on device tensors (fyprt_render_rays_device).  `rays`: contiguous float32 (N, 8) tensor on this context's GPU,
        one fyprt_ray per row; `pixel_indices`: None or a contiguous int32 (N,) tensor on the same GPU.  Returns a float32 (N, 4) tensor of
        radiance, and with `want_payload` also a float32 (N, 10) tensor of primary records (as trace_rays_tensor).  Ordered against
        torch's current stream as trace_rays_tensor is, without a host synchronisation and without record_stream."""
        import torch
        n = self._check_record_tensor("render_rays_tensor", "rays", rays, 8)
        if pixel_indices is not None:
            if pixel_indices.dtype != torch.int32 or pixel_indices.dim() != 1 or pixel_indices.shape[0] != n or not pixel_indices.is_contiguous():
                raise ValueError("render_rays_tensor: pixel_indices must be a contiguous int32 (N,) tensor, one per ray")
            if pixel_indices.device != rays.device:
                raise ValueError("render_rays_tensor: pixel_indices must be on the rays' GPU")
        rad = torch.empty((n, 4), dtype=torch.float32, device=rays.device)
        pay = torch.empty((n, 10), dtype=torch.float32, device=rays.device) if want_payload else None
        with self._on_context_stream(rays.device):
            self._check(self.lib.fyprt_render_rays_device(self.h, C.byref(settings), int(frame_index), C.c_void_p(rays.data_ptr()),
                                                          C.c_void_p(pixel_indices.data_ptr()) if pixel_indices is not None else None,
                                                          int(first_index), n, C.c_void_p(rad.data_ptr()),
                                                          C.c_void_p(pay.data_ptr()) if pay is not None else None))
        return (rad, pay) if want_payload else rad

    def denoise(self, params: DenoiseParams | None = None, want_radiance=True, with_stats=False):
        """Edge-avoiding denoise of the frame rendered last (fyprt_denoise, blocking; defaults when `params` is None).  Returns
        (image H x W uint32 ABGR8, radiance H x W x 4 float32 or None without `want_radiance`), with `with_stats` also the FrameStats of
        the call.  No frame state moves; read_buffer(BUF_ALBEDO) afterwards gives the albedo guide of that frame."""
        p = params if params is not None else DenoiseParams()
        return _denoise_blocking(self, self, "fyprt_denoise", (C.byref(p),), None, want_radiance, FrameStats(), with_stats)

    def denoise_tensor(self, image_tensor, radiance_tensor, params: DenoiseParams | None = None):
        """Denoise into device tensors (fyprt_denoise_device): `image_tensor` a contiguous int32 (H, W) tensor or None, `radiance_tensor`
        a contiguous float32 (H, W, 4) tensor or None, on this context's GPU.  Ordered against torch's current stream as
        trace_rays_tensor is, without a host synchronisation and without record_stream."""
        p = params if params is not None else DenoiseParams()
        _denoise_tensor(self, self, "the context's GPU", "denoise_tensor", "fyprt_denoise_device", (C.byref(p),), 1, image_tensor, radiance_tensor)

    def denoise_temporal(self, params: TemporalParams | None = None, want_radiance=True, with_stats=False):
        """Temporal denoise of the frame rendered last (fyprt_denoise_temporal, blocking; defaults when `params` is None): reprojected
        history, per-pixel variance, variance-guided a-trous.  Returns as denoise() does.  No frame state moves; the context's history
        advances (read_buffer(BUF_TEMPORAL) gives the record written, denoise_temporal_reset() drops it)."""
        p = params if params is not None else TemporalParams()
        return _denoise_blocking(self, self, "fyprt_denoise_temporal", (C.byref(p),), None, want_radiance, FrameStats(), with_stats)

    def denoise_temporal_tensor(self, image_tensor, radiance_tensor, params: TemporalParams | None = None):
        """denoise_temporal into device tensors (fyprt_denoise_temporal_device); tensors and stream ordering exactly as denoise_tensor."""
        p = params if params is not None else TemporalParams()
        _denoise_tensor(self, self, "the context's GPU", "denoise_temporal_tensor", "fyprt_denoise_temporal_device", (C.byref(p),), 1, image_tensor, radiance_tensor)

    def denoise_upscale(self, params: UpscaleParams | None = None, want_radiance=True, with_stats=False):
        """Denoise the frame rendered last at its own size and present it at scale x that size (fyprt_denoise_upscale, blocking; defaults
        when `params` is None): the low-res stage of denoise() or, with params.temporal, of denoise_temporal() — the history then advances
        as in that call — hi-res primary rays, and a resolve guided by them.  Returns (image sH x sW uint32 ABGR8, radiance sH x sW x 4
        float32 or None), with `with_stats` also the FrameStats.  read_buffer(BUF_UPSCALE_GUIDE / BUF_UPSCALE_ALBEDO) afterwards gives the
        hi-res records (sH * sW of them)."""
        p = params if params is not None else UpscaleParams()
        out = _denoise_blocking(self, self, "fyprt_denoise_upscale", (C.byref(p),), int(p.scale), want_radiance, FrameStats(), with_stats)
        self._upscale = int(p.scale)
        return out

    def denoise_upscale_tensor(self, image_tensor, radiance_tensor, params: UpscaleParams | None = None):
        """denoise_upscale into device tensors of the hi-res size (fyprt_denoise_upscale_device): int32 (sH, sW) / float32 (sH, sW, 4);
        stream ordering exactly as denoise_tensor."""
        p = params if params is not None else UpscaleParams()
        _denoise_tensor(self, self, "the context's GPU", "denoise_upscale_tensor", "fyprt_denoise_upscale_device", (C.byref(p),), int(p.scale), image_tensor, radiance_tensor)
        self._upscale = int(p.scale)

    def denoise_temporal_reset(self):
        """Drops the temporal history (fyprt_denoise_temporal_reset): the next denoise_temporal* call behaves as a first call."""
        self._check(self.lib.fyprt_denoise_temporal_reset(self.h))

    def denoise_temporal_set_motion(self, on: bool):
        """Object motion for the temporal denoiser (fyprt_denoise_temporal_set_motion): with it on, update_vertices / update_transforms
        keep the history and the next denoise_temporal* call reprojects through the geometry of the frame denoised before.  A change of
        the mode drops the history."""
        self._check(self.lib.fyprt_denoise_temporal_set_motion(self.h, 1 if on else 0))

    def export_lighttrees(self, mesh_count: int):
        tc, tr, bt = C.c_uint32(), C.c_uint32(), C.c_uint32()
        first = np.zeros(mesh_count, dtype=np.uint32)
        count = np.zeros(mesh_count, dtype=np.uint32)
        root = np.zeros(mesh_count, dtype=np.uint32)
        self._check(self.lib.fyprt_export_lighttrees(self.h, None, C.byref(tc), C.byref(tr), None, C.byref(bt), None, None, None))
        tlas = np.zeros(tc.value, dtype=LT_NODE_DTYPE)
        blas = np.zeros(bt.value, dtype=LT_NODE_DTYPE)
        self._check(self.lib.fyprt_export_lighttrees(self.h, _ptr(tlas), C.byref(tc), C.byref(tr), _ptr(blas), C.byref(bt),
                                                     _ptr(first), _ptr(count), _ptr(root)))
        return {"tlas": tlas, "tlas_root": tr.value, "blas": blas, "blas_first": first, "blas_count": count, "blas_root": root}


def _u32_array(values):
    return (C.c_uint32 * len(values))(*[int(v) for v in values])


class Group:
    """Several contexts (one per GPU) of ONE process rendering one frame in row bands: fyprt_group_* (peer copies, no RCCL)."""

    def __init__(self, contexts, row_bounds, halo_mode=0):
        self.contexts, self.lib = list(contexts), contexts[0].lib
        arr = (C.c_void_p * len(contexts))(*[c.h for c in contexts])
        h = C.c_void_p()
        rc = self.lib.fyprt_group_create(arr, len(contexts), _u32_array(row_bounds), C.byref(h))
        if rc != 0:
            raise FyprtError(f"fyprt_group_create failed ({rc}): {self.lib.fyprt_last_error(contexts[0].h).decode()}")
        self.h, self.row_bounds = h, list(row_bounds)
        self.set_halo_mode(halo_mode)

    def _check(self, rc):
        if rc != 0:
            raise FyprtError(f"fyprt error {rc}: " + " | ".join(self.lib.fyprt_last_error(c.h).decode() for c in self.contexts))

    def set_halo_mode(self, mode):
        self._check(self.lib.fyprt_group_set_halo_mode(self.h, mode))

    def set_interleave(self, stripe_rows):
        self._check(self.lib.fyprt_group_set_interleave(self.h, stripe_rows))

    def set_rows(self, row_bounds):
        self._check(self.lib.fyprt_group_set_rows(self.h, _u32_array(row_bounds)))
        self.row_bounds = list(row_bounds)

    def render(self, settings):
        self._check(self.lib.fyprt_group_render(self.h, C.byref(settings)))

    def gather(self, root=0):
        self._check(self.lib.fyprt_group_gather(self.h, root))

    def synchronize(self):
        self._check(self.lib.fyprt_group_synchronize(self.h))

    def denoise(self, params: DenoiseParams | None = None, want_radiance=True, with_band_ms=False):
        """Context.denoise for the frame the group rendered last, every band filtered by its owner (fyprt_group_denoise, blocking;
        defaults when `params` is None).  Returns (image H x W uint32 ABGR8, radiance H x W x 4 float32 or None without `want_radiance`)
        of the WHOLE frame, bit for bit a single context's; with `with_band_ms` also the per-band milliseconds of the call."""
        p = params if params is not None else DenoiseParams()
        return _denoise_blocking(self, self.contexts[0], "fyprt_group_denoise", (C.byref(p),), None, want_radiance, (C.c_float * len(self.contexts))(), with_band_ms)

    def _denoise_tensor(self, who, fn, args, scale, root, image_tensor, radiance_tensor):
        if not 0 <= root < len(self.contexts):
            raise ValueError(f"{who}: root out of range")
        _denoise_tensor(self, self.contexts[root], "the root context's GPU", who, fn, args + (root,), scale, image_tensor, radiance_tensor)

    def denoise_tensor(self, image_tensor, radiance_tensor, params: DenoiseParams | None = None, root=0):
        """Context.denoise_tensor for the group (fyprt_group_denoise_device): the tensors live on the GPU of context `root`, and the call
        is ordered against torch's current stream through that context's stream, without a host synchronisation."""
        p = params if params is not None else DenoiseParams()
        self._denoise_tensor("denoise_tensor", "fyprt_group_denoise_device", (C.byref(p),), 1, root, image_tensor, radiance_tensor)

    def denoise_temporal(self, params: TemporalParams | None = None, history_rows=GROUP_HISTORY_ROWS, want_radiance=True, with_band_ms=False):
        """Context.denoise_temporal for the frame the group rendered last (fyprt_group_denoise_temporal, blocking; defaults when `params`
        is None): every band reprojects into the group's history — its own rows and `history_rows` rows either side, the band's history
        window — and filters its rows.  Returns as denoise() does.  With history_rows >= height the sequence is a single context's."""
        p = params if params is not None else TemporalParams()
        return _denoise_blocking(self, self.contexts[0], "fyprt_group_denoise_temporal", (C.byref(p), int(history_rows)), None, want_radiance,
                                 (C.c_float * len(self.contexts))(), with_band_ms)

    def denoise_temporal_tensor(self, image_tensor, radiance_tensor, params: TemporalParams | None = None, history_rows=GROUP_HISTORY_ROWS, root=0):
        """denoise_temporal into device tensors on the GPU of context `root` (fyprt_group_denoise_temporal_device); tensors and stream
        ordering exactly as denoise_tensor."""
        p = params if params is not None else TemporalParams()
        self._denoise_tensor("denoise_temporal_tensor", "fyprt_group_denoise_temporal_device", (C.byref(p), int(history_rows)), 1, root, image_tensor, radiance_tensor)

    def denoise_upscale(self, params: UpscaleParams | None = None, history_rows=GROUP_HISTORY_ROWS, want_radiance=True, with_band_ms=False):
        """Context.denoise_upscale for the frame the group rendered last (fyprt_group_denoise_upscale, blocking; defaults when `params` is
        None): the low-res stage of denoise() or, with params.temporal, of denoise_temporal() with `history_rows` on the bands, then every
        band traces and resolves its own hi-res rows.  Returns (image sH x sW uint32 ABGR8, radiance sH x sW x 4 float32 or None) of the
        WHOLE frame, with `with_band_ms` also the per-band milliseconds.  Afterwards read_buffer(BUF_UPSCALE_GUIDE / BUF_UPSCALE_ALBEDO)
        of a member gives its hi-res records, valid in the hi-res rows of its band."""
        p = params if params is not None else UpscaleParams()
        out = _denoise_blocking(self, self.contexts[0], "fyprt_group_denoise_upscale", (C.byref(p), int(history_rows)), int(p.scale), want_radiance,
                                (C.c_float * len(self.contexts))(), with_band_ms)
        for c in self.contexts:
            c._upscale = int(p.scale)
        return out

    def denoise_upscale_tensor(self, image_tensor, radiance_tensor, params: UpscaleParams | None = None, history_rows=GROUP_HISTORY_ROWS, root=0):
        """denoise_upscale into device tensors of the hi-res size on the GPU of context `root` (fyprt_group_denoise_upscale_device): int32
        (sH, sW) / float32 (sH, sW, 4); stream ordering exactly as denoise_tensor."""
        p = params if params is not None else UpscaleParams()
        self._denoise_tensor("denoise_upscale_tensor", "fyprt_group_denoise_upscale_device", (C.byref(p), int(history_rows)), int(p.scale), root, image_tensor, radiance_tensor)
        for c in self.contexts:
            c._upscale = int(p.scale)

    def denoise_temporal_reset(self):
        """Drops every member's temporal history (fyprt_group_denoise_temporal_reset): the next denoise_temporal* call is a first call."""
        self._check(self.lib.fyprt_group_denoise_temporal_reset(self.h))

    def close(self):
        if getattr(self, "h", None):
            self.lib.fyprt_group_destroy(self.h)
            self.h = None


def live_device_bytes(lib=None) -> int:
    """fyprt_live_device_bytes: device bytes the library's buffers hold right now, over every context of the process."""
    return int((lib or load_library()).fyprt_live_device_bytes())


def balance_rows(row_bounds, band_ms, min_rows=16, max_shift=1 << 30, lib=None):
    """fyprt_balance_rows: cost-balanced band boundaries from the per-band frame times."""
    lib = lib or load_library()
    n = len(band_ms)
    out = (C.c_uint32 * (n + 1))()
    rc = lib.fyprt_balance_rows(_u32_array(row_bounds), (C.c_float * n)(*[float(x) for x in band_ms]), n, min_rows, max_shift, out)
    if rc != 0:
        raise FyprtError(f"fyprt_balance_rows failed ({rc})")
    return list(out)


def comm_ops(kind, row_bounds, rank, width, bytes_per_pixel, halo=0, height=0, wrap_row=True, new_bounds=None, lib=None):
    """fyprt_comm_ops: [(is_recv, peer, buffer, offset, bytes), ...] that `rank` issues in one RCCL group section (kind 0: halo exchange,
    kind 1: fyprt_comm_set_rows from row_bounds to new_bounds)."""
    lib = lib or load_library()
    n = len(row_bounds) - 1
    nb = _u32_array(new_bounds) if new_bounds is not None else None
    args = (kind, _u32_array(row_bounds), nb, n, halo, height, 1 if wrap_row else 0, width, rank, _u32_array(bytes_per_pixel), len(bytes_per_pixel))
    cnt = lib.fyprt_comm_ops(*args, None, 0)
    if cnt < 0:
        raise FyprtError("fyprt_comm_ops: bad arguments")
    out = (C.c_uint64 * (5 * max(cnt, 1)))()
    lib.fyprt_comm_ops(*args, out, cnt)
    return [tuple(int(v) for v in out[5 * k: 5 * k + 5]) for k in range(cnt)]


def halo_plan(row_bounds, halo, height, wrap_row=True, lib=None):
    """fyprt_halo_plan: [(receiver, owner, first row, end row), ...] of one halo exchange."""
    lib = lib or load_library()
    n = len(row_bounds) - 1
    cnt = lib.fyprt_halo_plan(_u32_array(row_bounds), n, halo, height, 1 if wrap_row else 0, None, 0)
    out = (C.c_uint32 * (4 * max(cnt, 1)))()
    lib.fyprt_halo_plan(_u32_array(row_bounds), n, halo, height, 1 if wrap_row else 0, out, cnt)
    return [tuple(out[4 * k: 4 * k + 4]) for k in range(cnt)]


def _export_plan(lib, fn, row_bounds, *args):
    """A fyprt_group_denoise*_plan entry `fn`: asked for the number of entries, then for the entries, as (stage, receiver, owner, first
    row, end row) tuples."""
    f = getattr(lib or load_library(), fn)
    args = (_u32_array(row_bounds), len(row_bounds) - 1) + args
    cnt = f(*args, None, 0)
    if cnt < 0:
        raise FyprtError(f"{fn} failed ({cnt})")
    out = (C.c_uint32 * (5 * max(cnt, 1)))()
    f(*args, out, cnt)
    return [tuple(out[5 * k: 5 * k + 5]) for k in range(cnt)]


def group_denoise_plan(row_bounds, height, iterations, lib=None):
    """fyprt_group_denoise_plan: [(stage, receiver, owner, first row, end row), ...] of one Group.denoise call, in issue order."""
    return _export_plan(lib, "fyprt_group_denoise_plan", row_bounds, height, iterations)


def group_denoise_temporal_plan(row_bounds, height, iterations, history_rows=GROUP_HISTORY_ROWS, lib=None):
    """fyprt_group_denoise_temporal_plan: [(stage, receiver, owner, first row, end row), ...] of one Group.denoise_temporal call that finds a
    history, in issue order (stage 0 guides, 1 prepared colour, 2 history, 3 + k colour and variance of iteration k)."""
    return _export_plan(lib, "fyprt_group_denoise_temporal_plan", row_bounds, height, iterations, history_rows)


def group_denoise_upscale_plan(row_bounds, height, iterations, temporal=False, history_rows=GROUP_HISTORY_ROWS, lib=None):
    """fyprt_group_denoise_upscale_plan: [(stage, receiver, owner, first row, end row), ...] of one Group.denoise_upscale call, in issue
    order: the plan of the low-res stage (group_denoise_plan, or with `temporal` group_denoise_temporal_plan), then the stage that brings
    every band but the last the colour row below it."""
    return _export_plan(lib, "fyprt_group_denoise_upscale_plan", row_bounds, height, iterations, 1 if temporal else 0, history_rows)
