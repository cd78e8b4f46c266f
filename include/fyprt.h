/*
 * fyprt.h — C ABI of the MI355X-native trace + shade path (libfyprt.so).
 *
 * This is the drop-in boundary for ONE path of Savasstion/FYPRayTracer: everything
 * `Renderer::Render` does between "scene/camera are on the host" and "RGBA8 + float4
 * accumulation are back on the host" (reference: FYPRayTracer/src/Classes/Core/Renderer.cu:13-284
 * and the 11 __global__ kernels it launches, Renderer.cu:2431-2900).  Plain pointers and sizes
 * only; no C++, HIP or torch types cross this boundary.  Each entry point cites the
 * reference interface it replaces.  The reference-side binding a maintainer would add is
 * shown in INTEGRATION.md.
 *
 * Error convention: every call returns FYPRT_OK (0) or a negative FYPRT_E* code and
 * records a message retrievable with fyprt_last_error().  (The reference prints
 * cudaGetErrorString to stderr and keeps going, Renderer.cu:29-47; the C++ facade in
 * fypraytracer_amd/host/ reproduces that on top of these codes.)
 *
 * Threading: one context per host thread and per GPU; a context owns one HIP stream.
 */
#ifndef FYPRT_H
#define FYPRT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FYPRT_OK 0
#define FYPRT_EINVAL (-1)   /* bad argument / inconsistent scene description            */
#define FYPRT_EHIP (-2)     /* a HIP runtime call failed (message has hipGetErrorString) */
#define FYPRT_ESTATE (-3)   /* call order violated (render before resize/scene/camera)   */
#define FYPRT_ENOLIGHT (-4) /* light-based technique on a scene with no emissive triangle
                               (the reference reads out of bounds there)                 */

/* SamplingTechniqueEnum.h:4-17 — values fixed by the reference's enum order. */
enum fyprt_technique {
    FYPRT_BRUTE_FORCE = 0,
    FYPRT_UNIFORM_SAMPLING = 1,
    FYPRT_COSINE_WEIGHTED_SAMPLING = 2,
    FYPRT_GGX_SAMPLING = 3,
    FYPRT_BRDF_SAMPLING = 4,
    FYPRT_LIGHT_SOURCE_SAMPLING = 5,
    FYPRT_NEE = 6,
    FYPRT_RESTIR_DI = 7,
    FYPRT_RESTIR_GI = 8
};

/* RenderingSettings.h:5-22 — field-for-field, 52 bytes, so the reference's struct can be
 * passed by address (bool == 1 byte + padding under both the MSVC x64 and SysV ABIs). */
typedef struct fyprt_settings {
    uint8_t to_accumulate;          /* toAccumulate */
    uint8_t _pad0[3];
    int32_t light_bounces;          /* lightBounces   (cast to uint8_t by the kernels, Renderer.cu:2444) */
    int32_t sample_count;           /* sampleCount    (cast to uint8_t, Renderer.cu:2480-2481)            */
    float sky_color[3];             /* skyColor */
    int32_t technique;              /* currentSamplingTechnique (enum fyprt_technique) */
    int32_t light_candidate_count;  /* lightCandidateCount */
    uint32_t rand_seed;             /* randSeed */
    uint8_t use_temporal_reuse;     /* useTemporalReuse */
    uint8_t use_spatial_reuse;      /* useSpatialReuse */
    uint8_t _pad1[2];
    int32_t temporal_history_limit; /* temporalHistoryLimit   (cast to uint8_t, Renderer.cu:1775) */
    int32_t spatial_neighbor_num;   /* spatialNeighborNum     (cast to uint8_t, Renderer.cu:1896) */
    int32_t spatial_neighbor_radius;/* spatialNeighborRadius  (cast to uint8_t, Renderer.cu:1897) */
} fyprt_settings;

/* Vertex.h:5-10 (32 B): world-space vertices, i.e. Scene::worldVertices (Scene.cpp:42-51). */
typedef struct fyprt_vertex { float position[3]; float normal[3]; float uv[2]; } fyprt_vertex;

/* Material.cuh:7-16 (44 B).  is_use_albedo_map overlays the reference's `bool` + 3 padding
 * bytes: only the low byte is read. */
typedef struct fyprt_material {
    uint32_t is_use_albedo_map;
    float albedo[3];
    uint32_t albedo_map_index;
    float roughness, metallic;
    float emission_color[3];
    float emission_power;
} fyprt_material;

/* Mesh.h:26-31 reduced to what the path reads: the triangle range of the mesh inside
 * Scene::triangles (indexStart/3, indexCount/3) and its material. */
typedef struct fyprt_mesh { uint32_t first_triangle, triangle_count; int32_t material_index; } fyprt_mesh;

/* Texture.cuh:9-14: ABGR8 pixels (A<<24|B<<16|G<<8|R), row-major. */
typedef struct fyprt_texture { const uint32_t* pixels; uint32_t width, height; } fyprt_texture;

/* LightTree.cuh:28-49 flattened (plain floats, explicit centroid because the reference's
 * UnionAABB leaves inner-node centroids at the origin, AABB.cuh:43-57). 80 bytes. */
typedef struct fyprt_lighttree_node {
    float energy;
    uint32_t num_emitters;
    uint32_t left;            /* Node::offset       (left child, inner nodes)                   */
    uint32_t right_or_emitter;/* Node::emitterIndex (right child | triangle index | mesh index) */
    uint32_t is_leaf;
    float cone_axis[3], theta_o, theta_e;   /* bounds_o */
    float box_lo[3], box_hi[3], box_centroid[3]; /* bounds_w */
    uint32_t _pad;
} fyprt_lighttree_node;

/* Optional prebuilt light trees in the reference's own shape (Scene::lightTree_tlas +
 * Mesh::lightTree_blas).  If `tlas_nodes` is NULL the library builds them itself with its
 * restatement of LightTree.cpp:21-293 (needed only by LIGHT_SOURCE_SAMPLING and NEE). */
typedef struct fyprt_lighttrees {
    const fyprt_lighttree_node* tlas_nodes; uint32_t tlas_node_count, tlas_root;
    const fyprt_lighttree_node* blas_nodes;  /* all per-mesh trees concatenated              */
    const uint32_t* blas_first;              /* [mesh_count] first node of mesh m's tree     */
    const uint32_t* blas_count;              /* [mesh_count] node count (0 = mesh not a light)*/
    const uint32_t* blas_root;               /* [mesh_count] root index relative to blas_first*/
} fyprt_lighttrees;

/* What SceneToGPU deep-copies (Scene_GPU.cpp:6-81), as flat arrays + counts. */
typedef struct fyprt_scene_desc {
    const fyprt_vertex* vertices; uint32_t vertex_count;          /* Scene::worldVertices */
    const void* triangles; uint32_t triangle_count; uint32_t triangle_stride;
        /* Scene::triangles: each record starts with {uint32 v0,v1,v2; int32 materialIndex}
           (Triangle.cuh:9-10); stride 52 passes the reference's array as is, 16 a packed one. */
    const fyprt_material* materials; uint32_t material_count;     /* Scene::materials */
    const fyprt_mesh* meshes; uint32_t mesh_count;                /* Scene::meshes    */
    const fyprt_texture* textures; uint32_t texture_count;        /* Scene::textures  */
    const uint32_t* emissive_triangles; uint32_t emissive_count;  /* Scene::emissiveTriangles; NULL = derive
                                                                     as InitSceneEmissiveTriangles, Scene.cpp:209-221 */
    const fyprt_lighttrees* light_trees;                          /* may be NULL */
} fyprt_scene_desc;

/* What CameraToGPU uploads (Camera_GPU.cu:4-60) minus the W*H ray-direction array, which is
 * regenerated on the device from inverse_projection / inverse_view with the arithmetic of
 * Camera::RecalculateRayDirections (Camera.cpp:136-153).  Matrices are column-major float[16]
 * exactly as glm::mat4 stores them. */
typedef struct fyprt_camera_desc {
    float projection[16], view[16], prev_projection[16], prev_view[16];
    float inverse_projection[16], inverse_view[16];
    float position[3];
    uint32_t viewport_width, viewport_height;
} fyprt_camera_desc;

typedef struct fyprt_context fyprt_context;

/* Per-frame statistics of the last fyprt_render call. */
typedef struct fyprt_frame_stats {
    float kernel_ms;        /* hipEvent time over the frame's kernels on the context stream */
    float kernel_ms_part[4];/* per launch (trace/shade, DI/GI part 1, part 2, ...), 0 if unused */
    uint64_t rays;          /* TraceRay invocations            } only with fyprt_set_ray_counting(ctx, 1):    */
    uint64_t box_tests;     /* AABB slab tests executed        } the SURVEY.md §8(d) instrumentation, exact    */
    uint64_t tri_tests;     /* ray/triangle tests executed     } per-lane counts reduced with device atomics   */
    uint64_t hits;          /* rays that found a triangle      }                                               */
    uint64_t part_rays[4], part_box_tests[4], part_tri_tests[4], part_hits[4];   /* the same, per launch */
    uint32_t launches;
    uint64_t node_visits;   /* 64-byte node records fetched (one per visit; box_tests counts the valid children tested in them) */
    uint64_t part_node_visits[4];
} fyprt_frame_stats;

/* Buffers readable with fyprt_read_buffer (device -> host, for parity tests). */
enum fyprt_buffer {
    FYPRT_BUF_ACCUM = 0,        /* float4 running sum          (Renderer.h:21 m_AccumulationData) */
    FYPRT_BUF_IMAGE = 1,        /* uint32 ABGR8                (Renderer.h:20 m_RenderImageData)  */
    FYPRT_BUF_PAYLOAD = 2,      /* RayHitPayload 40 B          (Renderer.h:31)                    */
    FYPRT_BUF_DEPTH = 3,        /* float                       (Renderer.h:29)                    */
    FYPRT_BUF_NORMAL = 4,       /* float2 octahedral, the frame just rendered (Renderer.h:30)     */
    FYPRT_BUF_DI_RESERVOIR = 5, /* ReSTIR_DI_Reservoir 20 B, after Part 1 (Renderer.h:34)         */
    FYPRT_BUF_DI_PREV = 6,      /* ... written by Part 2       (Renderer.h:35)                    */
    FYPRT_BUF_GI_RESERVOIR = 7, /* ReSTIR_GI_Reservoir 72 B    (Renderer.h:38)                    */
    FYPRT_BUF_GI_PREV = 8,      /*                             (Renderer.h:39)                    */
    FYPRT_BUF_ALBEDO = 9,       /* float4: rgb = albedo of the primary hit, w = 1 filterable / 0 not (rgb 0 there); written by
                                   fyprt_denoise* for the frame it denoised, FYPRT_ESTATE before (new, no reference counterpart) */
    FYPRT_BUF_TEMPORAL = 10,    /* 64 B: P.xyz, t | n.xyz, filterable | colour.rgb, N | m1, m2, variance, 0 — the history record the last
                                   fyprt_denoise_temporal* call wrote; FYPRT_ESTATE before the first call and after anything that drops the
                                   history (new, no reference counterpart) */
    FYPRT_BUF_UPSCALE_GUIDE = 11,  /* 32 B per HI-RES pixel (scale*width x scale*height of the last fyprt_denoise_upscale* call): P.xyz, t |
                                   n.xyz, filterable (1.0 / 0.0) — the denoiser's guide record of the hi-res primary hit; FYPRT_ESTATE
                                   before the first successful call and after fyprt_resize (new, no reference counterpart) */
    FYPRT_BUF_UPSCALE_ALBEDO = 12  /* float4 per hi-res pixel, valid as the guide: rgb = albedo, w = 1 for a filterable pixel; rgb = the
                                   pass-through colour (sky / emission), w = 0 otherwise */
};

/* ---- lifetime (the reference has none: Renderer owns raw pointers and never frees them,
 *      Renderer.cu:421-457 FreeDynamicallyAllocatedMemory is never called) */
int fyprt_create(int device_ordinal, fyprt_context** out);
void fyprt_destroy(fyprt_context* ctx);
const char* fyprt_last_error(const fyprt_context* ctx);   /* ctx may be NULL: last create error */

/* Renderer::OnResize + ResizeReservoirs/DepthBuffers/NormalBuffers/PrimaryHitPayloadBuffers
 * (Renderer.cpp:5-41, Renderer.cu:286-419): (re)allocates and zero-fills every per-pixel
 * buffer and resets the frame index to 1.  Unlike the reference the device buffers exist
 * after the FIRST call (Renderer.cpp:24-27 skips them). */
int fyprt_resize(fyprt_context* ctx, uint32_t width, uint32_t height);

/* Multi-GPU tile split (new; BASELINE.json north_star): this context renders image rows
 * [row_begin,row_end) of the full width x height frame.  ReSTIR Part 1 is additionally run
 * on `halo_rows` rows either side (halo recompute).  Default: all rows.  With spatial reuse on, halo_rows must be
 * at least spatial_neighbor_radius (or the rows must arrive by fyprt_group_* / fyprt_comm_* exchange): what a neighbour beyond
 * band + halo holds is whatever an earlier frame left there. */
int fyprt_set_rows(fyprt_context* ctx, uint32_t row_begin, uint32_t row_end, uint32_t halo_rows);
/* The interleaved split of SURVEY.md §8(e) for the techniques whose pixels are independent (every technique but the two ReSTIRs:
 * PerPixel_* of Renderer.cu:565-1626 read nothing of another pixel): the frame is cut into stripes of `stripe_rows` rows and this
 * context renders the stripes part, part + parts, part + 2 parts, ... — every part samples the whole image, so the parts cost the
 * same without balancing.  stripe_rows 0 returns to the rows of fyprt_set_rows.  A ReSTIR frame on a striped context fails with
 * FYPRT_ESTATE (spatial reuse reads the rows around a pixel).  Pixel values do not depend on the split. */
int fyprt_set_row_stripes(fyprt_context* ctx, uint32_t stripe_rows, uint32_t parts, uint32_t part);

/* SceneToGPU / FreeSceneGPU (Scene_GPU.cpp:6-163) + Renderer::SetSceneToBeUpdatedFlag(true)
 * (Renderer.h:56): builds the acceleration structure and uploads everything. */
int fyprt_upload_scene(fyprt_context* ctx, const fyprt_scene_desc* scene);

/* CameraToGPU (Camera_GPU.cu:4-60), called by Renderer::Render every frame (Renderer.cu:70). */
int fyprt_set_camera(fyprt_context* ctx, const fyprt_camera_desc* camera);

/* Renderer::Render (Renderer.cu:13-284): one frame with the given settings: selects the
 * technique's kernel(s) (Renderer.cu:87-235), accumulates, tonemaps and packs on the device,
 * then advances the frame index (Renderer.cu:258-261).  Blocking. `stats` may be NULL. */
int fyprt_render(fyprt_context* ctx, const fyprt_settings* settings, fyprt_frame_stats* stats);

/* Asynchronous variant: enqueues the frame on the context's stream and returns. */
int fyprt_render_async(fyprt_context* ctx, const fyprt_settings* settings);
int fyprt_synchronize(fyprt_context* ctx);
/* Per-launch hipEvent times (ms) of the frame enqueued `frames_back` frames ago (0 = the last one; the last 128 frames
 * are kept).  The events are recorded on the context's streams by both render variants; call after fyprt_synchronize.
 * A ReSTIR DI frame reports three parts (launches == 3).  Pipelined with Part 1 split (tuning key 21, asynchronous frames): part 0 =
 * the primary kernel (primary rays + light candidates, between its own events on its own stream), part 1 = the temporal kernel + the
 * setup kernel on the front stream, part 2 = the trace kernel.  Otherwise: part 0 = Part 1, part 1 = setup, part 2 = trace.  The parts of
 * a pipelined frame run beside parts of its neighbours: their sum is not the frame's time. */
int fyprt_frame_timings(fyprt_context* ctx, uint32_t frames_back, float* kernel_ms_part4, uint32_t* launches);

/* The D2H copies at Renderer.cu:244-250: rgba8 = m_RenderImageData (ABGR8, row 0 = NDC y -1),
 * accum4 = m_AccumulationData (float4 running SUM).  Either may be NULL.  Full frame size;
 * rows outside this context's band are left untouched. */
int fyprt_readback(fyprt_context* ctx, uint32_t* rgba8, float* accum4);

/* Device pointer of the ABGR8 image (width*height uint32) for an on-device gather (RCCL). */
int fyprt_image_device_ptr(fyprt_context* ctx, void** dptr);
/* Render into a caller-owned device image buffer (e.g. a torch tensor) instead of the internal one. */
int fyprt_set_external_image(fyprt_context* ctx, void* device_ptr);
/* The context's hipStream_t (as void*) so a caller can order its own work after a frame. */
int fyprt_stream(fyprt_context* ctx, void** stream);

int fyprt_read_buffer(fyprt_context* ctx, int which /* enum fyprt_buffer */, void* dst, size_t bytes);

/* The geometry moved, the topology did not (a transform edit through SceneManager::PerformAllSceneUpdates,
 * SceneManager.cpp:24-66, where the reference rebuilds the mesh's BLAS, the TLAS and the light trees on the host): the new world
 * vertices (same count and order as uploaded) refresh the per-triangle records, the leaf triangles and the boxes of the
 * acceleration structure ON THE DEVICE; the tree keeps its shape (fyprt_upload_scene rebuilds it).  Light records are rebuilt by
 * their kernel, the light trees on the host.  Not available for scenes uploaded with prebuilt light trees. */
int fyprt_update_vertices(fyprt_context* ctx, const fyprt_vertex* vertices, uint32_t vertex_count);

/* A material edit — SceneManager::PerformAllSceneUpdates with materialsToUpdate / meshMatToBeUpdated (SceneManager.cpp:10-17, :69-85),
 * WalnutApp.cpp:702-723: a material's albedo, roughness, metallic, emission, texture switch or index changed, a mesh got another material,
 * a material was created.  `materials` is the WHOLE table and replaces the uploaded one (material_count may be larger than the uploaded
 * count, never smaller); every listed mesh gets material_index = mesh_materials[k], and so do ALL its triangles (SceneManager.cpp:75-79);
 * `emissive_triangles` is read as the scene description's (NULL = derive).  Afterwards the context is in the state fyprt_upload_scene reaches
 * with the edited description — every later frame, query, exported light tree and emissive list is bit-identical — except that the
 * acceleration structure is NOT touched (fyprt_export_bvh returns the same bytes, a refitted tree included).  On the device: the 48-byte
 * material records, the reassigned triangles' material index, the emissive list (an ordered compaction: ascending triangle order, as
 * upload derives it) and the light records; the light trees are rebuilt on the host.  An edit that moves no emission (no material's
 * emission colour or power changed bit-wise, no reassigned mesh with an emissive old or new material, the emissive list derived as
 * before or handed over unchanged) only writes the table and the reassigned triangles.
 * Frame index, accumulation, reservoirs and ReSTIR history are kept, as upload keeps them; the last frame is no longer denoisable and the
 * temporal history is dropped.  Blocking: pipelined frames are waited for first, everything the call launches is complete on return.
 * Errors, in this order: FYPRT_EINVAL for a NULL context, NULL materials with a non-zero count, a NULL mesh array with mesh_count > 0,
 * material_count below the current count, a mesh index out of range, a material index < 0 or >= material_count, an emissive triangle
 * index >= the triangle count; FYPRT_ESTATE before fyprt_upload_scene and on a scene uploaded with prebuilt light trees.  Host-only
 * contexts are supported (everything but the device work).  A later render call answers FYPRT_ENOLIGHT as after an upload when the
 * edit leaves no emitter.  The scene is per context: call it on every member of a group or communicator between frames. */
int fyprt_update_materials(fyprt_context* ctx, const fyprt_material* materials, uint32_t material_count,
                           const uint32_t* mesh_indices, const int32_t* mesh_materials, uint32_t mesh_count,
                           const uint32_t* emissive_triangles, uint32_t emissive_count);
/* "Import Mesh" — WalnutApp.cpp:668-693 -> Scene::CreateNewMeshInScene (Scene.cpp:241-290) on Scene::AddNewMeshToScene (Scene.cpp:9-92):
 * vertices, triangles and mesh records are pushed onto the end of the scene's arrays, nothing that exists moves.  `vertices` are the NEW world
 * vertices, which follow the uploaded ones; `triangles` the NEW triangles (records as in fyprt_scene_desc), whose vertex indices are ABSOLUTE,
 * into the combined vertex array, as AddNewMeshToScene offsets them by vertexStart; `meshes` the NEW meshes with ABSOLUTE first_triangle,
 * which must partition the triangle range [T_old, T_old + triangle_count) in order.  `object_vertices`: NULL, or vertex_count object-space
 * vertices with `mesh_first_vertex`, mesh_count + 1 ABSOLUTE entries from V_old to V_old + vertex_count: the object-space copy and the mesh
 * vertex ranges of fyprt_set_object_vertices are extended under its checks, so fyprt_update_transforms works on old and new meshes (a
 * context that holds no copy ignores them); with NULL a copy the context holds is released, as fyprt_upload_scene releases it.
 * Afterwards the context is in the state fyprt_upload_scene reaches with the combined description, bit for bit — every per-triangle record,
 * the material table (untouched), the exported light trees and emissive list, the light records, every later frame, ray query and radiance
 * query (checked by an oracle that walks the exported tree) — except for the acceleration structure.  The emissive list is the old list,
 * explicit or derived, followed by the appended triangles whose material emits, in ascending order: for a derived list exactly what upload
 * derives for the combined scene.  Frame index, accumulation, reservoirs and ReSTIR history are kept, as upload keeps them; the last frame is no
 * longer denoisable; the temporal history and the motion snapshot are dropped, as upload drops them.
 * Acceleration structure — the graft: a sub-tree is built over the appended triangles only, with the builder of tuning key 12 (0: the host
 * builder over the new meshes; 1, 2: the device LBVH / PLOC builder over the triangle range from five triangles on, otherwise the host
 * builder); its nodes are appended to the node array and its leaf records to the leaf-triangle array.  With S the sub-tree's root (a leaf
 * code when the append has few triangles) and R the current root: an inner R with fewer than four children takes S as child[count];
 * otherwise (R is full, or a leaf code) a new two-child node (R, S) is appended as the LAST node and becomes the root; an empty tree
 * becomes S.  The level count of R / the new root stays exact.  Apart from R when it takes the child (its grid is quantised again), every
 * old node and every old leaf record keeps its index and its bytes.  Boxes and quantisation of the new nodes and of R / the new root come
 * from the refit pass run over those nodes only; a host-only context quantises R / the new root with the host builder's quantiser from R's
 * grid origin and its conservative upper planes.  The tree grows by one level about every third append; when the result would exceed 31
 * levels or the node index range, the call rebuilds the tree of the combined scene as fyprt_upload_scene would.
 * fyprt_set_append_placement(ctx, 1) links S at the cheapest place by a surface-area cost instead of the root (below).
 * Cost: of the old scene only the per-node level grouping (4 bytes per node) crosses the bus; the scene's device arrays have a capacity that at
 * least doubles when exceeded and move device to device (fyprt_live_device_bytes counts the capacity); per-triangle records, emissive list
 * (an ordered compaction over the appended range), light records and the refit run on the device; the light trees of the new emissive meshes
 * and the TLAS are built on the host.  An append without an emitter leaves the lights alone; its per-triangle and per-mesh light tables grow
 * on the device like the scene's arrays, so that they cover the combined scene (a removal writes them in place and keeps their capacity).
 * Blocking: pipelined frames are waited for first, everything the call launches is complete on return.  Errors, in this order: FYPRT_EINVAL
 * for a NULL context, a NULL array with a non-zero count (or object_vertices without mesh_first_vertex), triangle_stride < 16, a vertex index
 * >= the combined vertex count, a material index outside the current table, meshes that do not partition the appended range in order,
 * mesh_first_vertex out of order or not spanning [V_old, V_old + vertex_count], a triangle outside its mesh's vertex range (with
 * object_vertices only); FYPRT_ESTATE before fyprt_upload_scene and on a scene uploaded with prebuilt light trees.  triangle_count == 0 &&
 * mesh_count == 0 returns FYPRT_OK and changes nothing.  Host-only contexts are supported (everything but the device work).  The scene is
 * per context: call it on every member of a group or communicator between frames. */
int fyprt_append_meshes(fyprt_context* ctx,
                        const fyprt_vertex* vertices, uint32_t vertex_count,
                        const void* triangles, uint32_t triangle_count, uint32_t triangle_stride,
                        const fyprt_mesh* meshes, uint32_t mesh_count,
                        const fyprt_vertex* object_vertices, const uint32_t* mesh_first_vertex);
/* Where fyprt_append_meshes links the sub-tree.  New (no reference counterpart).  mode 0 (default): at the root, the graft above, byte for
 * byte.  mode 1: at the cheapest place by a surface-area cost.  A graft at the root makes every ray test the import's box, and every third
 * import puts a level on top of the whole scene; mode 1 puts a small import next to what it lies in.
 * The placement rule.  All arithmetic is IEEE binary32, every operation rounded on its own, no fma contraction, on the device and on the host.
 *   B       exact box of the appended triangles' world vertices
 *   b(Y)    exact box of inner node Y (the union of its triangles' vertices); a leaf child's exact box likewise
 *   A(b)    with d = hi - lo per axis: (d.x*d.y + d.y*d.z) + d.z*d.x
 *   U(a,b)  per-axis min and max
 *   g(Y)    A(U(b(Y), B)) - A(b(Y))                                      (>= 0 exactly: rounding is monotone)
 *   P(X)    acc = g(X); acc = acc + g(parent); acc = acc + g(grandparent); ... up to the root, in that order
 *   d(X)    number of ancestors of X;   h = level count of the sub-tree's root S (0 when S is a leaf code)
 * Candidates, for every inner node X of the old tree:
 *   slot              count(X) < 4     cost P(X)                          hX = max(levels(X), h + 1)
 *   pair with child i i < count(X)     cost P(X) + A(U(b(child_i), B))    hX = max(levels(X), hN + 1), hN = 1 + max(levels(child_i), h),
 *                                                                         levels 0 for a leaf child
 *   root pair         once per tree    cost A(U(b(R), B))                 new root levels 1 + max(levels(R), h)
 * A slot or pair candidate is feasible iff d(X) + hX <= 31, the root pair iff its new root levels are <= 31; the node total must stay below
 * 2^24; a candidate whose cost is not finite is skipped.  The winner is the minimum of the 64-bit key (cost bits << 32) | id, with
 * id = node * 8 + i for a pair, node * 8 + 4 for a slot, 0xFFFFFFFF for the root pair: a cost tie goes to the lowest id, the root pair loses
 * every tie.  No feasible candidate: the rebuild fall-back of mode 0.  An empty tree or a root that is a leaf code follows mode 0's rule.
 * Link: the sub-tree's nodes and leaf records go behind the old ones as in mode 0.  A pair's new node N is the LAST node, its children
 * (old child, S) in that order.  In X only the one slot changes; the slot order of the other children is kept (exact-t ties depend on it).
 * The level counts of N, X and every ancestor stay exact (1 + max over the inner children); they get box and quantisation from the refit of
 * one node, lowest first (a host-only context quantises them as a removal does).  Every other old node and every old leaf record keeps its
 * index and its bytes.  Apart from the acceleration structure the state equals fyprt_upload_scene of the combined scene bit for bit, as
 * mode 0 promises.
 * Cost over mode 0: the parent links of the tree are built (as the first partial refit builds them; the append invalidates them again), one
 * search launch with one thread per inner node, 16 bytes back (the key and the candidate count), and the path's refit in one launch.  The
 * search's scratch (16 bytes) is counted by fyprt_live_device_bytes.
 * Errors: FYPRT_EINVAL for a NULL context or a mode other than 0 or 1. */
int fyprt_set_append_placement(fyprt_context* ctx, int mode);
typedef struct fyprt_append_placement {
    uint32_t mode;          /* mode in effect for that append */
    uint32_t kind;          /* 0 first (tree was empty or a leaf code: mode 0's rule)
                               1 slot: S is child[count] of node
                               2 pair: new last node (child[slot] of node, S) replaces that child
                               3 root pair: new last node (R, S) is the root
                               4 rebuilt: no feasible place, tree rebuilt as upload builds it */
    uint32_t node, slot, depth;      /* depth = ancestors of node; all 0 for kinds 0, 3, 4 */
    uint32_t cost_bits;              /* the winning cost as binary32 bits; 0 in mode 0, for kinds 0 and 4 and for a leaf-code root */
    uint32_t levels_before, levels_after, candidates;   /* candidates = feasible, finite ones (0 where no search ran) */
} fyprt_append_placement;
/* The report of the last successful fyprt_append_meshes with triangles, in either mode (mode 0: kinds 0, 1 at the root, 3 and 4).  Errors, in
 * this order: FYPRT_EINVAL for NULL arguments; FYPRT_ESTATE before the first such append. */
int fyprt_last_append_placement(fyprt_context* ctx, fyprt_append_placement* out);
/* Mesh removal, applied ON THE DEVICE.  New (no reference counterpart: the reference can import a mesh but not delete one).  The meshes
 * `mesh_indices` (mesh_count distinct indices, any order) leave the scene.  Reduced description: the listed mesh records are gone and later
 * meshes move down; their triangle ranges are gone, surviving triangles keep their relative order (new index = old index - removed triangles
 * before it) and surviving meshes' first_triangle shifts likewise; the vertex ranges given are gone, surviving vertices keep their order and
 * surviving triangles' vertex indices shift likewise.  `vertex_ranges`: NULL, or 2 * mesh_count words, (first, count) per listed mesh.  With
 * NULL a context that holds the object-space copy (fyprt_set_object_vertices / an append with object vertices) removes each listed mesh's
 * own range [mesh_first_vertex[m], mesh_first_vertex[m + 1]); a context without the copy removes no vertex, and the orphaned vertices stay
 * part of the description.  Given ranges on a context that holds the copy must be exactly the meshes' own.  The object-space copy and
 * mesh_first_vertex are compacted with the rest, so fyprt_update_transforms and fyprt_update_vertices go on working with the reduced arrays.
 * Materials and textures are untouched.
 * Afterwards the context is in the state fyprt_upload_scene reaches with the reduced description, bit for bit — every per-triangle record,
 * the exported light trees and emissive list, the light records, every later frame, ray query and radiance query (checked by an oracle that
 * walks the exported tree) — except for the acceleration structure.  The emissive list is the old one, explicit or derived, minus the removed
 * triangles, remapped and kept in order: for a derived list exactly what upload derives.  Frame index, accumulation, reservoirs and ReSTIR
 * history are kept, as upload keeps them (a history light index beyond the shorter list is rejected by the temporal pass); the last frame is
 * no longer denoisable; the temporal history and the motion snapshot are dropped, as an append drops them.  A later light-based render
 * answers FYPRT_ENOLIGHT when no emitter is left; removing every mesh leaves the state of an upload of a scene without triangles.
 * Acceleration structure — the prune rule: the tree is pruned bottom-up, never rebuilt (a removal cannot deepen it).
 *   Leaf records: a record whose triangle is removed is dead; the array is compacted stably; survivors keep every byte except the triangle
 *     index, which is remapped.  One record per triangle holds again.
 *   Leaf codes: (first, n) becomes (first - dead records before first, survivors in the range); with no survivor the child is dead.
 *   Nodes, by level, levels = 1 first: a node's surviving children — remapped leaf codes and the replacements of inner children — are
 *     compacted stably (slot order is kept, so exact-t ties resolve as before).  No survivor: the node is dead.  Exactly one: the node is
 *     dead and is replaced in its parent by that survivor (a splice; chains collapse).  Two or more: the node lives with the new count and
 *     levels = 1 + max(levels of its inner children).  The root follows the same rule: it may become a leaf code, or empty.
 *   Node array: compacted stably (the area ordering survives), inner references rebased; node boxes and the level grouping follow.
 *   Boxes: a node that lost no triangle anywhere below it keeps all bytes except rebased references.  Every other surviving node gets its
 *     box and quantisation from the refit pass run over just those nodes, lowest level first (after exact boxes for a tree no refit has run
 *     on); a host-only context quantises them with the host builder's quantiser from the children's exact lower corners and conservative
 *     upper planes and exact leaf boxes.
 * Cost: nothing per triangle crosses the bus.  Every stream is compacted on the device into a buffer of the same capacity (capacities are
 * kept: a removal never grows fyprt_live_device_bytes beyond its value before the call, and a later append of the same size fits without
 * growing); 4 bytes per leaf record come back (the dead counts, from which the host repeats the node pass on its topology copy), the range
 * tables, the refit list and the level grouping (4 bytes per node) go up; light records by their kernel, light trees on the host.
 * Blocking: pipelined frames are waited for first, everything the call launches is complete on return.  Errors, in this order: FYPRT_EINVAL
 * for a NULL context, NULL mesh_indices with a non-zero count, a mesh index out of range, a mesh listed twice, a vertex range beyond the
 * vertex count, two vertex ranges that overlap, with an object-space copy held a range that is not the mesh's own, a surviving triangle that
 * uses a removed vertex; FYPRT_ESTATE before fyprt_upload_scene and on a scene uploaded with prebuilt light trees.  A failed call changes
 * nothing.  mesh_count == 0 returns FYPRT_OK and changes nothing.  Host-only contexts are supported (everything but the device work).  The
 * scene is per context: call it on every member of a group or communicator between frames. */
int fyprt_remove_meshes(fyprt_context* ctx, const uint32_t* mesh_indices, uint32_t mesh_count,
                        const uint32_t* vertex_ranges /* NULL, or 2 * mesh_count: (first, count) per listed mesh */);
/* Regraft: the listed meshes are taken out of the tree and linked in again where they lie NOW.  New (no reference counterpart).  The
 * geometry edits (fyprt_update_transforms, fyprt_update_vertices, fyprt_update_mesh_vertices) refit boxes only: a mesh that was moved across
 * the scene keeps its leaf records under the nodes of its old neighbourhood, every ancestor's box spans both places and every ray through
 * the gap visits them.  This call repairs the tree without fyprt_upload_scene: nothing but the tree moves.  `mesh_indices`: mesh_count
 * distinct mesh indices; `reports`: NULL, or mesh_count entries.
 * 1. Tree-only prune.  The prune rule of fyprt_remove_meshes, exactly as stated there, with this dead set: every leaf record whose triangle
 *    lies in a listed mesh's range [first_triangle, first_triangle + triangle_count).  No triangle leaves the scene, so no triangle is
 *    renumbered: surviving leaf records keep EVERY byte.  Leaf codes, the node pass by level, splices, the stable compaction of the node array,
 *    rebased references, the refit of just the nodes that lost something and the level grouping are a removal's.
 * 2. One graft per listed mesh, in the order listed: the graft of fyprt_append_meshes for that mesh's triangle range, as if the mesh had
 *    just been appended.  Sub-tree by the builder of tuning key 12 (the device builders from five triangles on, otherwise the host builder);
 *    the device builders' Morton grid is the exact box B of the mesh's triangles (the box of the vertices an append would have passed when the
 *    mesh uses all of its vertices).  The sub-tree's nodes go behind the old nodes, its leaf records behind the old records (the record array
 *    ends at the triangle count again), linked by the placement mode in effect (fyprt_set_append_placement: 0 at the root, 1 at the cheapest
 *    place); the new nodes and the path are refitted as in an append.  reports[k] is the fyprt_append_placement of the graft of
 *    mesh_indices[k].  A graft that answers "rebuild" (too deep, node range) rebuilds the whole tree as fyprt_upload_scene builds it: this
 *    and every remaining report then say kind 4.  A listed mesh without triangles is skipped, its report is zero apart from `mode`.  After
 *    device transform edits the host's vertex copy is refreshed from the device first, as fyprt_append_meshes refreshes it.
 * 3. Nothing else moves: the per-triangle and per-vertex streams, materials, the emissive list, light records and light trees, the
 *    object-space copy, frame index, accumulation, reservoirs and ReSTIR history, fyprt_last_append_placement and fyprt_last_edit_stats are
 *    untouched.  The last frame stays denoisable; the temporal history and a pending motion snapshot are kept (the payload's triangle indices
 *    and every world position are what they were).  Only the partial refit's parent links are invalidated.  Every later frame and query
 *    equals the one before the call bit for bit, except where two triangles are hit at exactly the same t — the promise of any valid tree.
 * Consequence: the tree after the call is the tree of a twin context that removed the listed meshes in ONE fyprt_remove_meshes and appended
 * them again, one call each in the listed order, under the same tuning key 12 and placement mode: nodes64 equal byte for byte, tris48 equal
 * in every byte except triangleIndex, which maps through the twin's renumbering, and reports[k] equal to the twin's
 * fyprt_last_append_placement after its k-th append.  (The device builders hand out node indices by atomic counters, so two builds of one
 * tree differ in the numbering of their nodes and leaf records: with tuning key 12 = 1 or 2 "equal" is up to that numbering.)
 * Memory: the prune compacts into buffers of the same capacity and frees its scratch; the kept scratch of an append (graft list, parent
 * links, search result) is left at the size it had.  fyprt_live_device_bytes returns to its value before the call unless the regrafted
 * tree has more nodes than the node arrays' capacity, which then at least doubles as in an append.
 * Blocking: pipelined frames are waited for first, everything the call launches is complete on return.  Errors, in this order: FYPRT_EINVAL
 * for a NULL context, NULL mesh_indices with a non-zero count, a mesh index out of range, a mesh listed twice; FYPRT_ESTATE before
 * fyprt_upload_scene.  Scenes with prebuilt light trees are allowed (the light trees are not touched).  A failed check changes nothing.
 * mesh_count == 0 returns FYPRT_OK and changes nothing.  Host-only contexts are supported (everything but the device work).  The scene is
 * per context: regraft the members of a group or communicator one by one between frames. */
int fyprt_regraft_meshes(fyprt_context* ctx, const uint32_t* mesh_indices, uint32_t mesh_count,
                         fyprt_append_placement* reports /* NULL, or mesh_count entries */);
/* Surface-area cost of the tree as it is.  New (no reference counterpart).  Reads the tree, changes nothing: what tells an application that
 * a moved mesh should be regrafted.  A, b(Y) and the exact leaf boxes are those of the placement rule above: A in binary32, every operation
 * rounded on its own, no contraction; exact boxes from the triangles' world vertices.  Each term is converted to binary64 and summed in
 * binary64.  (inner_area + leaf_area) / root_area is the usual SAH estimate; the caller forms it.
 * On a device one thread per node computes the terms, workgroups reduce them in a fixed order into one pair of sums each, and the host adds
 * the pairs in workgroup order: no floating-point atomics, so two calls on the same tree return the same bits.  A host-only context adds the
 * same terms in node order; the two agree within 2^-26 relative (at most 2^26 non-negative terms: any summation order is within
 * (n - 1) * 2^-53 <= 2^-27 relative of the exact sum).  The partial sums' buffer (16 bytes per 256 nodes) is kept and counted by
 * fyprt_live_device_bytes; a tree no refit has run on gets the pass that fills every node's exact box first.
 * Blocking: pipelined frames are waited for first.  Errors, in this order: FYPRT_EINVAL for NULL arguments; FYPRT_ESTATE before
 * fyprt_upload_scene. */
typedef struct fyprt_tree_cost_sums {
    double root_area;      /* (double) A(b(R)); of a leaf-code root its exact leaf box; 0 for an empty tree */
    double inner_area;     /* sum over inner nodes Y of (double) A(b(Y)) */
    double leaf_area;      /* sum over leaf children (first, n) of n * (double) A(exact box of those n triangles); a leaf-code root counts
                              as the one leaf child */
    uint32_t nodes, leaf_children, leaf_records, levels;
} fyprt_tree_cost_sums;
int fyprt_tree_cost(fyprt_context* ctx, fyprt_tree_cost_sums* out);
/* "Import Texture" — WalnutApp.cpp:739-754 -> Scene::CreateNewTextureInScene (Scene.cpp:228-239): the new pixel arrays are uploaded and the
 * texture table is extended; old pixel buffers stay where they are.  The context is then, bit for bit, one that uploaded the scene with the
 * longer list.  Acceleration structure, frame state and temporal history are untouched and the last frame stays denoisable — unless a
 * material's albedo_map_index already pointed at one of the new slots (indices beyond the table shade as solid colour): then the last frame
 * is no longer denoisable and the temporal history is dropped, as after fyprt_update_materials.  Blocking.  Errors: FYPRT_EINVAL for a NULL
 * context, NULL textures with a non-zero count, an empty or NULL texture; FYPRT_ESTATE before fyprt_upload_scene.  count == 0 changes nothing. */
int fyprt_append_textures(fyprt_context* ctx, const fyprt_texture* textures, uint32_t count);
/* The emissive-triangle list in effect (Scene::emissiveTriangles as uploaded, derived or updated).  NULL `triangles` queries the count. */
int fyprt_export_emissive(fyprt_context* ctx, uint32_t* triangles, uint32_t* count);

/* Renderer::ResetFrameIndex / GetCurrentFrameIndex (Renderer.h:47,49). */
int fyprt_reset_frame_index(fyprt_context* ctx);
uint32_t fyprt_frame_index(const fyprt_context* ctx);

/* Export of the library's own acceleration structure as plain arrays, so an
 * instrumented CPU restatement of the same traversal can count box / triangle tests
 * (SURVEY.md §8d).  Call with NULL pointers to query the counts.
 *   nodes64: 64-byte 4-wide nodes { float origin[3]; uint8 ex[3], count; int32 child[4]; uint8 qlo[3][4], qhi[3][4]; uint32 pad[2] }
 *            child plane on axis a = origin[a] + q * 2^(ex[a]-127); child >= 0 inner node, < 0 leaf: ~child = firstTri << 2 | (n-1)
 *   tris48 : 48-byte leaf triangles { float v0[3], e1[3], e2[3]; uint32 triangleIndex; uint32 pad[2] }
 *   max_stack: worst-case number of pending traversal-stack entries of an ordered traversal (<= 31 by construction). */
int fyprt_export_bvh(fyprt_context* ctx, void* nodes64, uint32_t* node_count, void* tris48,
                     uint32_t* tri_count, int32_t* root_ref, uint32_t* max_stack);
/* Export of the light trees the library built (same flat node format as the input). */
int fyprt_export_lighttrees(fyprt_context* ctx, fyprt_lighttree_node* tlas, uint32_t* tlas_count, uint32_t* tlas_root,
                            fyprt_lighttree_node* blas, uint32_t* blas_total, uint32_t* blas_first,
                            uint32_t* blas_count, uint32_t* blas_root);

/* Count rays / box tests / triangle tests on the device (atomics; slows the frame); off by default. */
int fyprt_set_ray_counting(fyprt_context* ctx, int enabled);

/* Performance knobs (A/B experiments; defaults are the measured best).  Keys 0-7, 9-11 never change a result; keys 8 and 12
 * change the traversal order / the tree and with it only which of two triangles hit at EXACTLY the same t wins.
 * key 0: tile order — 0 linear, 1 one contiguous eighth of the tiles per XCD, 2 every 8th tile row per XCD.
 * key 1: ReSTIR DI Part 2 — 0 one thread per pixel, 1 setup kernel + shadow-task queue + persistent trace waves.
 * key 2: persistent workgroups per CU for the trace kernel (default 0 = as many as LDS and registers allow: 6 today).
 * key 3: 1 = counting-sort the shadow tasks by light bin before tracing (histogram matrix + column scan + scatter; one
 *        global atomic per setup workgroup, as without the sort).  Default 0: measured +0.04 ms for the sort and no faster trace — shadow-ray cost is
 *        dominated by the geometry around the ray ORIGIN, which the unsorted tile order already keeps coherent.
 * key 4: tasks a persistent wave claims per queue-head atomic (default 128).
 * key 5: idle lanes that trigger a refill of a persistent wave (default 24).
 * key 6: inner-node loop quorum of the ReSTIR DI Part-2 shadow-ray kernels and the path engine's ray kernels: lanes waiting at a leaf are
 *        served once fewer than this many lanes are still walking inner nodes (default 24; 0 = classic while-while).  The count is for a full
 *        wave; r03: a wave in which only some lanes still have a ray scales it to those lanes (rt_device.h: quorum_of).
 * key 7: the same for the kernels that trace primary rays (k_primary, k_gi_primary, ReSTIR DI Part 1, the fused small-scene frame):
 *        default 32 since r03 (bench frame 0.843 -> 0.82-0.83 ms, config 3 3.09 -> 3.03 ms; it was neutral before the node visit was trimmed); 0 = never.
 * key 8: pending-entry budget of the traversal stack rule (default 0 = a few entries above the tree's level count, chosen
 *        so that one more workgroup fits a CU's LDS; at most 31; always clamped from below to the tree's level count):
 *        siblings are pushed one by one while pending + 2 + levels(node) <= budget, else as one resume entry; the LDS stack holds budget + 1 entries per thread.
 *        Unlike keys 0-7 the value can change the visiting order (exact-t ties may resolve differently).
 * key 9: chunks every persistent wave owns statically before it starts stealing from the shared head (default 0 = auto: 2 — r03: bench frame
 *        0.833 -> 0.820 ms, config 3 3.13 -> 3.08 ms against 1; on queues shorter than the grid the static part is an even share and no atomic is issued at all).
 * key 10: smallest chunk of the guided self-scheduling of the shared part: claims shrink from key 4 towards this value as
 *        the queue runs out (default 32).
 * key 11: 1 (default) = wavefront ReSTIR DI frames are pipelined over two streams (three with key 21): Part 1 + setup of frame N+1 run beside the
 *        trace kernel of frame N (asynchronous frames only overlap, of course; a blocking fyprt_render waits for its frame).
 * key 12: builder of the acceleration structure for the NEXT fyprt_upload_scene: 0 (default) host binned SAH + SAH-optimal
 *        collapse; 1 device LBVH (Morton sort, Karras radix tree, collapse, refit) — milliseconds instead of a fraction of a
 *        second for a million triangles, a tree 1.65x slower to trace; 2 device PLOC (Morton sort, parallel locally-ordered
 *        clustering with search radius FYPRT_PLOC_RADIUS = 16, collapse, refit) — the same build time, a tree 1.15x slower to
 *        trace than the host builder's.  Both fall back to the host builder if the tree gets deeper than 31 wide levels.
 *        Results stay exact in every case (any valid tree finds the same closest hits but for exact-t ties).
 * key 13: MEASUREMENT ONLY (tools/band_rate.py): 1 = a lone context skips ReSTIR Part 1 on its halo rows as a band does in halo-exchange
 *        mode, without anybody filling them — the cost of one band of an exchange-mode split; the image near the band border is not valid.
 * key 14: 1 = ReSTIR DI Part-2 setup fetches every neighbour record the spatial-reuse loop can possibly visit at once (the addresses
 *        depend only on how many earlier neighbours were accepted) instead of one dependent gather per neighbour; same results.
 *        Default 0: measured slower (0.259 vs 0.225 ms) — register pressure and request rate outweigh the saved round trips.
 *        2 = the reservoir neighbourhood's hot fields (depth, normal; 12 B) of the workgroup's 76 x 76 pixel window staged in LDS (69 KB),
 *        the geometry test served from there; same results; measured slower as well (profiles/README.md r02).
 * key 15: ray kernel of the wavefront stages (techniques 0-6, ReSTIR GI): 1 = persistent waves with lane refill, 2 = one thread per ray,
 *        0 (default) = by tree size: one thread per ray below 65 536 triangles, where rays are too cheap for the refill machinery to pay.
 * key 16: EXPERIMENT, acts only in a -DRT_TOPCACHE build: the first N nodes of the (area-ordered) node array are also kept in LDS by the
 *        ReSTIR DI traversal kernels (0..1024).  Measured a net loss (profiles/README.md r03); compiled out by default.
 * key 17: techniques 0-5 on a tree of fewer than 65 536 triangles render the whole frame in ONE launch (k_path_fused: one thread per pixel,
 *        the stage path's step functions): 0 (default) = by tree size, 1 = always the stages, 2 = always fused.  Same results.
 * key 18: 1 (default) = a ReSTIR DI Part-2 shadow ray whose pixel is black in EVERY outcome (both candidate radiances exactly zero) is
 *        not traced; 0 = every Part-2 pixel traces its ray as Renderer.cu:2010-2031 does.  Same pixels; fewer rays are counted.
 *        Also on by default since r03: key 2 = 0 uses at most 4 workgroups per CU for the persistent ReSTIR DI grid while frames are pipelined.
 * key 19: ReSTIR GI Part 2.  2 (default) = ONE persistent launch (k_gi2_persistent): a lane owns a pixel of the Part-2 list for its whole neighbour
 *         loop — reservoir state in registers, visibility rays traced in place — and the lanes of a wave that have no ray in flight are serviced
 *         together (merge the verdict, next accepted neighbour, next pixel from the list), like the persistent trace kernels' refill.
 *         0 = the stages (2 x neighbours + 1 launches; state, ray and result records move through memory).  1 = one launch, one thread per
 *         pixel without refill (slower on a whole frame, kept for comparison).  Same pixels bit for bit, same ray counts in every mode.
 * key 20: k_gi2_persistent (key 19 = 2): lanes of a wave without a ray in flight before the wave services them together (default 48; 0 = default).
 * key 21: 1 (default) = Part 1 of a pipelined ReSTIR DI frame (key 11, asynchronous frames) runs as two kernels: its history-free half (primary ray,
 *         material, light candidates) on a third stream — beside the previous frame's setup kernel, which writes the history — and the temporal
 *         merge on the front stream, fed through a private staging set per frame parity (72 B per pixel and parity).  0 = one kernel on the front
 *         stream.  Same results bit for bit; blocking, instrumented and two-call frames always take the one kernel.
 * key 22: path of fyprt_update_transforms: 0 (default) = the full passes (every per-triangle record, every leaf record, every node of every
 *         level); 1 = the partial refit (below, fyprt_update_mesh_vertices): records and nodes of the listed meshes only.  Same state
 *         on a tree a full refit has run on; otherwise nodes and records nothing moved under keep their bytes.
 * key 25: 1 (default) = a ReSTIR DI frame keeps the primary hits while camera and geometry stand still: a pixel's primary payload depends on the
 *         camera's inverse projection, inverse view, position and viewport and on the geometry alone (no jitter, no seed, no material), so a
 *         frame whose rows (fyprt_set_rows: band, and band + halo) and camera fields equal, byte for byte, those of the ReSTIR DI frame that traced the payload in place reads it
 *         instead of tracing 1 ray per pixel again.  Every geometry, transform, topology or tree edit, fyprt_upload_scene, fyprt_resize, a changed
 *         tuning value and a frame of any other technique drop it (the next ReSTIR DI frame traces); material and texture edits keep it.
 *         Instrumented frames (fyprt_set_ray_counting) always trace, and count as ever.  0 = every frame traces.  Same results bit for bit;
 *         fyprt_kept_primary_frames counts the frames that reused the payload.  Changing ANY key's value drops the kept hits once.
 * Values are range-checked (FYPRT_EINVAL): key 0: 0..2, keys 1, 3, 11, 13, 18, 21, 22, 25: 0..1, keys 12, 14, 15, 17, 19: 0..2, key 2: 0..16, keys 5, 6, 7, 20: 0..64,
 * key 8: 0..31, key 16: 0..1024; key 23 is reserved (0), key 24 is not assigned (every value is refused). */
int fyprt_set_tuning(fyprt_context* ctx, int key, int value);
/* The value in effect (key 8: the budget actually used for the uploaded scene, which an instrumented restatement of the
 * traversal must use too). */
int fyprt_get_tuning(fyprt_context* ctx, int key, int* value);
/* ReSTIR DI frames since fyprt_create that read the kept primary hits instead of tracing them (tuning key 25); 0 on a host-only context. */
int fyprt_kept_primary_frames(fyprt_context* ctx, uint64_t* frames);

/* Scene::vertices (object space) + every mesh's vertex range [mesh_first_vertex[m], mesh_first_vertex[m+1]) (Mesh::vertexStart /
 * vertexCount), kept on the device so that fyprt_update_transforms can apply a transform edit there.  After fyprt_upload_scene. */
int fyprt_set_object_vertices(fyprt_context* ctx, const fyprt_vertex* object_vertices, uint32_t vertex_count, const uint32_t* mesh_first_vertex);
/* A transform edit of `count` meshes — SceneManager::PerformAllSceneUpdates with meshTransformToBeUpdated (SceneManager.cpp:24-66),
 * i.e. Mesh::worldTransformMatrix (column-major glm::mat4, 16 floats per listed mesh) applied to the mesh's object-space vertices as
 * Scene.cpp:42-51 does (position / w; normal by the model matrix with w = 0, normalised).  64 bytes per mesh cross the bus; world
 * vertices, per-triangle records, tree boxes and light records are refreshed on the device, the light trees of the moved emissive
 * meshes (+ the TLAS) on the host.  Same result as fyprt_update_vertices with the host-computed world vertices. */
int fyprt_update_transforms(fyprt_context* ctx, const uint32_t* mesh_indices, const float* matrices16, uint32_t count);

/* Partial refit: new world vertices for the listed meshes only.  `vertices`: the meshes' own vertex ranges [mesh_first_vertex[m],
 * mesh_first_vertex[m+1]) (fyprt_set_object_vertices) concatenated in the order listed; vertex_count = their sum.  Afterwards the context
 * is in the state fyprt_update_vertices reaches with the full array (the given vertices in place, every other vertex as it is on the
 * device): world vertices, per-triangle records, leaf records, light records, exported light trees, every later frame and query are equal
 * bit for bit.  Tree: every node with a moved triangle anywhere below it has the bytes (and the exact box) the full refit writes; every
 * other node and leaf record keeps its bytes — so on a tree a full refit has run on, fyprt_export_bvh is byte for byte the full update's.
 * Cost: the listed vertex ranges cross the bus; on the device the listed meshes' triangles, their leaf records and the nodes above them
 * are rewritten (a walk from the moved triangles to the root, level by level), nothing else is read or written.  The object-space copy is
 * not touched: a later transform of the mesh starts from it again, as after fyprt_update_vertices.  Frame, denoiser and motion-snapshot
 * state follow fyprt_update_transforms; the light trees of listed emissive meshes (+ the TLAS) are rebuilt on the host.  Blocking.
 * Memory: the first partial edit after an upload, append or removal builds the way up the tree — 4 bytes per node, per leaf record and
 * per triangle — and the walk's scratch — 8 bytes per node + 128 bytes; both are kept (fyprt_live_device_bytes counts them) until the
 * topology changes again.  A tree no refit has run on also gets one pass that fills every node's exact box first.
 * Errors, in this order: FYPRT_EINVAL: NULL context, NULL array with a non-zero count.  FYPRT_ESTATE: before fyprt_upload_scene; without
 * the mesh vertex ranges of fyprt_set_object_vertices; scene with prebuilt light trees; host-only context.  FYPRT_EINVAL: mesh index out
 * of range; mesh listed twice; vertex_count not the sum of the ranges.  A failed call changes nothing; mesh_count == 0 returns FYPRT_OK
 * and changes nothing. */
int fyprt_update_mesh_vertices(fyprt_context* ctx, const uint32_t* mesh_indices, uint32_t mesh_count, const fyprt_vertex* vertices, uint32_t vertex_count);

/* What the last fyprt_update_vertices / fyprt_update_transforms / fyprt_update_mesh_vertices covered.  partial: 0 = the full passes
 * (the counts are the scene's triangles, leaf records and nodes, and the tree's levels), 1 = the partial refit (distinct triangles,
 * leaf records and nodes rewritten, and the level launches made).  FYPRT_ESTATE before the first geometry edit. */
typedef struct fyprt_edit_stats { uint32_t partial, triangles_refreshed, leaf_records_refreshed, nodes_refit, level_launches; } fyprt_edit_stats;
int fyprt_last_edit_stats(fyprt_context* ctx, fyprt_edit_stats* out);

/* MisUtils::ComputeMSE / ComputePSNR (MisUtils.cpp:118-157) of the current frame against a host reference image, reduced on the
 * device (exact integer sums: equals the host routine bit for bit); `flip_reference_rows` reads the reference vertically flipped as
 * ComputeMSE reads its BMP original.  The benchmark workflow of WalnutApp.cpp:826-876 without a read-back.  `psnr` may be NULL. */
int fyprt_compare_image(fyprt_context* ctx, const uint32_t* reference_rgba8, int flip_reference_rows, double* mse, double* psnr);
/* Self-test of the arithmetic contract: the library's short correctly rounded sqrt / 1/x / 1/sqrt(x) sequences (rt_math.h) against the
 * compiler's IEEE sequences on ALL 2^32 binary32 arguments each.  mismatches[3] (and, optionally, the smallest offending argument's bits)
 * in the order sqrt, reciprocal, reciprocal square root; all zero on a sound build.  New (no reference counterpart). */
int fyprt_selftest_math(fyprt_context* ctx, uint64_t* mismatches3, uint32_t* first_bad3 /* may be NULL */);

/* Self-test of the arithmetic contract, function by function: shading function `probe` evaluated on the device for `count` argument
 * records at `in`, one result record each to `out` (host memory both) — by the very inline functions the frame kernels call, so a test
 * can compare each with the CPU oracle bit for bit at arguments no rendered picture reaches.  New (no reference counterpart).
 * A record is an array of 32-bit words (f = binary32, u = uint32), tightly packed, record i at word i * words:
 *   probe                          input words                                         output words
 *   SINCOS                         1: x (f; valid for 0 <= x <= 2*pi + eps)            2: sin, cos
 *   ACOS, POW5                     1: x (f)                                            1: result (f)
 *   RND                            1: seed (u)                                         2: value (f), seed after (u)
 *   OCT_ENCODE                     3: v (f)                                            2: e (f)
 *   OCT_DECODE                     2: e (f)                                            3: v (f)
 *   PACK_ABGR                      4: r g b a (f)                                      1: ABGR word (u)
 *   UNPACK_ABGR                    1: ABGR word (u)                                    4: r g b a (f)
 *   EVAL_BRDF                      16: surface record (below)                          3: rgb (f)
 *   PDF_BRDF, PDF_GGX              16: surface record                                  1: pdf (f)
 *   SAMPLE_UNIFORM / _COSINE /     16: surface record (L unused)                       5: direction (3 f), pdf (f), seed after (u)
 *     _GGX / _BRDF
 *   DI_UPDATE                      4: candidate (u), w (f), pdf (f), seed (u)          7: the 20-byte reservoir after one update of an empty one
 *                                                                                         (index u, W f, pdf f, weightSum f, M u), accepted (u), seed after (u)
 *   SAMPLE_ALBEDO                  3: u (f), v (f), texture index (u)                  3: rgb (f); (-1, -1, -1) for an index past the scene's textures
 *   CLUSTER_IMPORTANCE,            23: shading point (3 f), one fyprt_lighttree_node   1: importance (f)
 *     CLUSTER_IMPORTANCE_GENERAL       (20 words)
 *   ASIN_KERNEL                    2: z (one binary64, low word first; 0 <= z <= 0.25)  2: the polynomial under acos (one binary64)
 * Surface record: N (3 f), V (3 f), L (3 f), albedo (3 f), metallic (f), roughness (f), seed (u), one unused word.
 * SAMPLE_ALBEDO reads the textures of the uploaded scene (fyprt_upload_scene / fyprt_append_textures; FYPRT_ESTATE without a scene).
 * CLUSTER_IMPORTANCE is the form the light-tree walk calls: it takes a shorter path when the boxes of all 64 records a wave holds
 * (records 64k .. 64k+63) have no extent along one axis; CLUSTER_IMPORTANCE_GENERAL is the all-corners path whatever the boxes.
 * FYPRT_EINVAL: unknown probe, NULL `in` / `out` with count > 0.  FYPRT_ESTATE: host-only context.  count == 0 launches nothing.
 * Waits for the context's pending work first; touches no frame state. */
enum fyprt_probe {
    FYPRT_PROBE_SINCOS = 0, FYPRT_PROBE_ACOS = 1, FYPRT_PROBE_POW5 = 2, FYPRT_PROBE_RND = 3, FYPRT_PROBE_OCT_ENCODE = 4, FYPRT_PROBE_OCT_DECODE = 5,
    FYPRT_PROBE_PACK_ABGR = 6, FYPRT_PROBE_UNPACK_ABGR = 7, FYPRT_PROBE_EVAL_BRDF = 8, FYPRT_PROBE_PDF_BRDF = 9, FYPRT_PROBE_PDF_GGX = 10,
    FYPRT_PROBE_SAMPLE_UNIFORM = 11, FYPRT_PROBE_SAMPLE_COSINE = 12, FYPRT_PROBE_SAMPLE_GGX = 13, FYPRT_PROBE_SAMPLE_BRDF = 14,
    FYPRT_PROBE_DI_UPDATE = 15, FYPRT_PROBE_SAMPLE_ALBEDO = 16, FYPRT_PROBE_CLUSTER_IMPORTANCE = 17, FYPRT_PROBE_CLUSTER_IMPORTANCE_GENERAL = 18,
    FYPRT_PROBE_ASIN_KERNEL = 19, FYPRT_PROBE_COUNT = 20
};
int fyprt_selftest_functions(fyprt_context* ctx, int probe, const void* in, uint32_t count, void* out);

/* ================================================================================================= batched ray queries
 * New (no reference counterpart): the caller's rays traced against the uploaded scene by the frames' traversal core, outside any frame —
 * picking (the mesh under a viewport pixel), visibility probes, bakes, and timing traversal on a fixed ray set ("Batched ray queries").
 * Acceptance: a triangle is accepted at distance t when the reference's Möller–Trumbore passes (including its own t > 1e-4), t > tmin
 * and t < tmax.  Directions need not be normalised; t is in units of the direction.
 *   FYPRT_QUERY_CLOSEST : one RayHitPayload (40 B, the FYPRT_BUF_PAYLOAD record) per ray — the nearest accepted triangle (exact-t ties:
 *                         the first one found in traversal order, as in the frame kernels), or hitDistance -1 / objectIndex -1.  With
 *                         tmin <= 1e-4 and tmax = +inf the record is bit-identical to the one a frame's primary kernel writes for the ray.
 *   FYPRT_QUERY_OCCLUDED: one uint32 per ray, 1 if any triangle is accepted, else 0 (traversal stops at the first one).
 * A ray with a non-finite origin / direction component, a NaN tmin / tmax or tmin >= tmax is answered as a miss (0) without traversal.
 * Errors: FYPRT_EINVAL for a NULL context, an unknown query kind, NULL rays / results with count > 0 (and, device entry, rays not
 * 16-byte or results not 8-byte aligned); FYPRT_ESTATE on a host-only context or before fyprt_upload_scene; count 0 returns FYPRT_OK
 * and launches nothing.
 * A query changes no frame state (frame index, accumulation, reservoirs, payload / image buffers, frame timings and counters): it has
 * its own counters and queue head, and the host entry's staging buffers are allocated on the first query and kept.  Queries run on the
 * context stream, after the geometry of the preceding upload / vertex / transform update.  The kernel (persistent waves with lane
 * refill, or one thread per ray on trees below 65 536 triangles) follows tuning key 15 as the path engine's ray kernels do. */
typedef struct fyprt_ray { float origin[3]; float tmin; float direction[3]; float tmax; } fyprt_ray;   /* 32 B, 16-B aligned on the device */
enum fyprt_query { FYPRT_QUERY_CLOSEST = 0, FYPRT_QUERY_OCCLUDED = 1 };
/* Host memory, blocking.  `results`: count x 40 B (closest) or count x uint32 (occluded).  `stats` may be NULL: kernel_ms = the hipEvent
 * time of the query launch, launches = 1; with ray counting on (fyprt_set_ray_counting) rays / box_tests / tri_tests / hits /
 * node_visits as a frame counts them, part_*[0] = the totals. */
int fyprt_trace_rays(fyprt_context* ctx, int query /* enum fyprt_query */, const fyprt_ray* rays, uint32_t count, void* results,
                     fyprt_frame_stats* stats);
/* Device memory of the context's GPU (rays: count x fyprt_ray; results as above), asynchronous on the context stream (fyprt_stream). */
int fyprt_trace_rays_device(fyprt_context* ctx, int query /* enum fyprt_query */, const void* rays, uint32_t count, void* results);

/* Ordered multi-hit query: the max_hits nearest accepted triangles per ray, in order ("Multi-hit queries") — picking through
 * an occluder, thickness and penetration probes, ordered layers, crossing counts.
 *   Acceptance  : as FYPRT_QUERY_CLOSEST — the Möller–Trumbore passes, t > tmin and t < min(tmax, FLT_MAX).
 *   Order       : every accepted hit has the 64-bit key (bits(t) << 32) | triangle; t > 1e-4, so the bit pattern of t orders as its value.
 *                 The answer for a ray is its max_hits smallest keys in ascending order: exact-t ties go to the lower triangle index.  The
 *                 answer does not depend on the tree, the builder or the visiting order.
 *   Record      : t, u, v as the ray/triangle test returns them (u, v: the barycentrics, not the payload's texture coordinates);
 *                 triangle: the scene triangle index (the payload's objectIndex).  Unused records are {-1.0f, 0xFFFFFFFF, 0, 0};
 *                 hit_counts[i] = the number of used records of ray i (hit_counts may be NULL).
 *   Continuation: with `after` (count records), a hit is accepted only if its key is greater than the key of after[i] (its u, v are
 *                 ignored); an after[i] with t < 0 — the unused record — means "this ray is finished": zero hits, no traversal.  So
 *                 passing each pass's LAST record per ray back in until every count is 0 enumerates all hits: none is skipped or
 *                 repeated, exact ties included (which tracing again with tmin = t cannot give: t > tmin skips a second triangle at that t).
 *   Invalid rays: as above — zero hits without traversal, counted as a ray with no tests.
 * Errors, in this order: FYPRT_EINVAL for a NULL context, max_hits 0 or above FYPRT_QUERY_MAX_HITS, NULL rays / hits with count > 0, and
 * (device entry) rays, after or hits not 16-byte or hit_counts not 4-byte aligned; FYPRT_ESTATE on a host-only context or before
 * fyprt_upload_scene; count 0 returns FYPRT_OK and launches nothing.
 * No frame state moves, as for fyprt_trace_rays: the query has its own counters and queue head, and the host entry's staging buffers
 * grow on demand and are kept.  The kernel follows tuning key 15 (and keys 4, 5, 6, 9, 10) as the other queries'; each lane keeps its
 * sorted list in LDS behind the traversal stack, 16 bytes per entry — with the deepest stack, 8 entries fill the 64 KB a workgroup may
 * have, which is why the cap is 8. */
#define FYPRT_QUERY_MAX_HITS 8
typedef struct fyprt_ray_hit { float t; uint32_t triangle; float u, v; } fyprt_ray_hit;   /* 16 B, 16-B aligned on the device */
/* Host memory, blocking.  `hits`: count x max_hits records, ray-major.  `stats` may be NULL; it is filled as fyprt_trace_rays fills it,
 * `hits` counting the rays with at least one record. */
int fyprt_trace_ray_hits(fyprt_context* ctx, const fyprt_ray* rays, const fyprt_ray_hit* after /* NULL or count */, uint32_t count,
                         uint32_t max_hits, fyprt_ray_hit* hits /* count x max_hits */, uint32_t* hit_counts /* NULL or count */,
                         fyprt_frame_stats* stats /* may be NULL */);
/* Device memory of the context's GPU, asynchronous on the context stream (fyprt_stream). */
int fyprt_trace_ray_hits_device(fyprt_context* ctx, const void* rays, const void* after, uint32_t count, uint32_t max_hits, void* hits,
                                void* hit_counts);

/* Nearest-point query: the max_hits closest triangles to each point, in order ("Nearest-point queries") — snapping a mesh
 * onto the surface next to it, clearance checks, the triangles within a brush radius, the unsigned distance to the scene.
 * Every operation below is rounded on its own in IEEE binary32 (no contraction), dot(a,b) = (a.x*b.x + a.y*b.y) + a.z*b.z.
 *   Distance    : for the point p and a leaf record (v0, e1, e2) as fyprt_export_bvh returns it (v1, v2 are never formed), Ericson's
 *                 closest point on a triangle in this order:
 *                   ap = p - v0;  d1 = dot(e1, ap);  d2 = dot(e2, ap)
 *                   if d1 <= 0 and d2 <= 0:                       (u, v) = (0, 0)
 *                   bp = ap - e1;  d3 = dot(e1, bp);  d4 = dot(e2, bp)
 *                   elif d3 >= 0 and d4 <= d3:                    (u, v) = (1, 0)
 *                   vc = d1*d4 - d3*d2
 *                   elif vc <= 0 and d1 >= 0 and d3 <= 0:         (u, v) = (d1 / (d1 - d3), 0)
 *                   cp = ap - e2;  d5 = dot(e1, cp);  d6 = dot(e2, cp)
 *                   elif d6 >= 0 and d5 <= d6:                    (u, v) = (0, 1)
 *                   vb = d5*d2 - d1*d6
 *                   elif vb <= 0 and d2 >= 0 and d6 <= 0:         (u, v) = (0, d2 / (d2 - d6))
 *                   va = d3*d6 - d5*d4;  a = d4 - d3;  b = d5 - d6
 *                   elif va <= 0 and a >= 0 and b >= 0:           w = a / (a + b); (u, v) = (1 - w, w)
 *                   else:                                         s = (va + vb) + vc; f = 1 / s; (u, v) = (vb * f, vc * f)
 *                   u = u < 0 ? 0 : (u > 1 ? 1 : u);  m = 1 - u;  v = v < 0 ? 0 : (v > m ? m : v)      (selects: a NaN stays a NaN)
 *                   diff = (ap - u*e1) - v*e2 per component;  distance2 = dot(diff, diff)
 *                 The final clamp is part of the contract: it keeps the answered point inside the record's triangle up to rounding,
 *                 whatever the region tests did on a sliver, and the traversal's conservative cull rests on that.
 *   Acceptance  : distance2 <= r2, r2 = min(max_distance * max_distance, FLT_MAX); a NaN or infinite distance2 (a degenerate record) is
 *                 therefore rejected.  With `after`, the key must also be greater than the key of after[i].
 *   Order       : every accepted triangle has the 64-bit key (bits(distance2) << 32) | triangle; distance2 >= +0, so the bit pattern
 *                 orders as the value.  The answer for a point is its max_hits smallest keys in ascending order: exact ties go to the
 *                 lower triangle index.  The answer does not depend on the tree, the builder or the visiting order.
 *   Record      : distance2, u, v as computed above — the closest point is (1-u-v) A + u B + v C of the caller's own vertices;
 *                 triangle: the scene triangle index.  Unused records are {-1.0f, 0xFFFFFFFF, 0, 0}; hit_counts[i] = the number of used
 *                 records of point i (hit_counts may be NULL).
 *   Continuation: as the multi-hit query's — an after[i] with distance2 < 0 (the unused record) finishes the point: zero hits, no
 *                 traversal.  Passing each pass's LAST record per point back in until every count is 0 enumerates every triangle within
 *                 max_distance exactly once, ties included: the radius query.
 *   Invalid points: a non-finite position component, a NaN max_distance or max_distance < 0 — zero hits without traversal, counted as a
 *                 query with no tests.
 * Errors, in this order: FYPRT_EINVAL for a NULL context, max_hits 0 or above FYPRT_QUERY_MAX_HITS, NULL points / hits with count > 0, and
 * (device entry) points, after or hits not 16-byte or hit_counts not 4-byte aligned; FYPRT_ESTATE on a host-only context or before
 * fyprt_upload_scene; count 0 returns FYPRT_OK and launches nothing.
 * No frame state moves: the query has its own counters, queue head and events, and the host entry's staging buffers grow on demand and
 * are kept.  The kernel follows tuning key 15 (and keys 4, 5, 6, 9, 10) as the other queries'; the per-lane list is the multi-hit
 * query's.  With ray counting on, stats reports rays = points, box_tests = the valid child boxes tested, tri_tests, hits = points with at
 * least one record, node_visits. */
typedef struct fyprt_point     { float position[3]; float max_distance; } fyprt_point;      /* 16 B, 16-B aligned on the device */
typedef struct fyprt_point_hit { float distance2; uint32_t triangle; float u, v; } fyprt_point_hit;   /* 16 B */
/* Host memory, blocking.  `hits`: count x max_hits records, point-major.  `stats` may be NULL; it is filled as fyprt_trace_ray_hits fills it. */
int fyprt_nearest_points(fyprt_context* ctx, const fyprt_point* points, const fyprt_point_hit* after /* NULL or count */, uint32_t count,
                         uint32_t max_hits, fyprt_point_hit* hits /* count x max_hits */, uint32_t* hit_counts /* NULL or count */,
                         fyprt_frame_stats* stats /* may be NULL */);
/* Device memory of the context's GPU, asynchronous on the context stream (fyprt_stream). */
int fyprt_nearest_points_device(fyprt_context* ctx, const void* points, const void* after, uint32_t count, uint32_t max_hits, void* hits,
                                void* hit_counts);

/* Box-overlap query: the triangles that touch each axis-aligned box [lo, hi], lowest indices first ("Box-overlap
 * queries") — the triangles in a region for an editor's marquee, a physics broad phase, a voxeliser, a spatial cache.
 * Every operation below is rounded on its own in IEEE binary32 (no contraction), dot(a,b) = (a.x*b.x + a.y*b.y) + a.z*b.z,
 * cross(a,b) = (a.y*b.z - b.y*a.z, a.z*b.x - b.z*a.x, a.x*b.y - b.x*a.y).  min and max are selects, min(a,b) = a < b ? a : b and
 * max(a,b) = a > b ? a : b, of three values min(min(x0, x1), x2); every comparison is written positively, so a NaN anywhere in a record
 * rejects it.
 *   Test        : for the box and a leaf record (v0, e1, e2) as fyprt_export_bvh returns it, the separating-axis test in this order:
 *                   1. v1 = v0 + e1;  v2 = v0 + e2                                                  (per component)
 *                   2. box axes, on the untranslated coordinates: for each axis a, mn / mx over v0.a, v1.a, v2.a:
 *                        require mn <= hi.a and mx >= lo.a                                           (the box is closed)
 *                   3. c = (lo + hi) * 0.5f;  h = (hi - lo) * 0.5f;  p_k = v_k - c
 *                   4. nine edge axes: for each f in (e1, e2 - e1, e2), mn / mx over s_0, s_1, s_2:
 *                        x: s_k = p_k.z*f.y - p_k.y*f.z;  r = h.y*|f.z| + h.z*|f.y|
 *                        y: s_k = p_k.x*f.z - p_k.z*f.x;  r = h.x*|f.z| + h.z*|f.x|
 *                        z: s_k = p_k.y*f.x - p_k.x*f.y;  r = h.x*|f.y| + h.y*|f.x|
 *                        require mn <= r and mx >= -r
 *                   5. plane: n = cross(e1, e2);  d = dot(n, p_0);  r = (h.x*|n.x| + h.y*|n.y|) + h.z*|n.z|
 *                        require d <= r and d >= -r
 *                 A zero-area record passes 4 and 5 with 0 <= 0: step 2 alone decides it.
 *   Acceptance  : every requirement holds and, with `after`, the triangle index is greater than after[i].
 *   Touching    : is decided by this rounded arithmetic.  A box that is the single point v0 of a record always accepts that record; a
 *                 box at the caller's own second vertex V1 may not, because the record holds v0 + fl(V1 - V0), not V1.
 *   Invalid box : on any axis !(lo <= hi), or lo + hi or hi - lo not finite — zero records without traversal, counted as a query with
 *                 no tests.  The pads are ignored.
 *   Order       : the records of box i are its max_hits smallest accepted triangle indices, ascending; unused slots are 0xFFFFFFFF.
 *                 hit_counts[i] = the number of used slots, totals[i] = the number of ALL accepted triangles, also those beyond max_hits
 *                 (the traversal visits them anyway).  Both may be NULL.  The answer does not depend on the tree, the builder or the
 *                 visiting order.
 *   Continuation: as the other list queries' — after[i] == 0xFFFFFFFF (the unused slot) finishes the box: zero records, total 0, no
 *                 traversal.  Passing each pass's LAST slot per box back in lists every triangle exactly once; totals[i] tells how
 *                 many are still to come, this pass included.
 * Errors, in this order: FYPRT_EINVAL for a NULL context, max_hits 0 or above FYPRT_OVERLAP_MAX_HITS, NULL boxes / triangles with
 * count > 0, and (device entry) boxes not 16-byte or after, triangles, hit_counts or totals not 4-byte aligned; FYPRT_ESTATE on a
 * host-only context or before fyprt_upload_scene; count 0 returns FYPRT_OK and launches nothing.
 * No frame state moves: the query has its own counters, queue head and events, and the host entry's staging buffers grow on demand and
 * are kept.  The kernel follows tuning key 15 (and keys 4, 5, 6, 9, 10) as the other queries'; each lane keeps its sorted list in LDS
 * behind the traversal stack, 4 bytes per entry — with the deepest stack, 32 entries fill the 64 KB a workgroup may have, which is why
 * the cap is 32.  With ray counting on, stats reports rays = boxes, box_tests = the valid child boxes tested, tri_tests, hits = boxes
 * with at least one record, node_visits. */
#define FYPRT_OVERLAP_MAX_HITS 32
typedef struct fyprt_box { float lo[3]; uint32_t pad0; float hi[3]; uint32_t pad1; } fyprt_box;   /* 32 B, 16-B aligned on the device */
/* Host memory, blocking.  `triangles`: count x max_hits indices, box-major.  `stats` may be NULL; it is filled as fyprt_nearest_points fills it. */
int fyprt_overlap_boxes(fyprt_context* ctx, const fyprt_box* boxes, const uint32_t* after /* NULL or count */, uint32_t count,
                        uint32_t max_hits, uint32_t* triangles /* count x max_hits */, uint32_t* hit_counts /* NULL or count */,
                        uint32_t* totals /* NULL or count */, fyprt_frame_stats* stats /* may be NULL */);
/* Device memory of the context's GPU, asynchronous on the context stream (fyprt_stream). */
int fyprt_overlap_boxes_device(fyprt_context* ctx, const void* boxes, const void* after, uint32_t count, uint32_t max_hits, void* triangles,
                               void* hit_counts, void* totals);

/* Triangle-overlap query: the scene triangles that cut each of the caller's triangles, lowest indices first (DESIGN.md §4,
 * "Triangle-overlap queries") — the narrow phase behind fyprt_overlap_boxes' broad phase: collision checks, interpenetration
 * highlighting, placement validation after an import, contact lists for a physics step.  Mask out the mesh in hand (query filters,
 * below) and query its triangles.
 * Every operation is rounded on its own in IEEE binary32 (no contraction); dot, cross, min / max as selects, min and max of three and
 * the positively written comparisons are exactly those of the box query above, so a NaN anywhere in a scene record rejects it.
 *   Test        : for the query triangle (q0, q1, q2) and a leaf record (v0, e1, e2) as fyprt_export_bvh returns it:
 *                   1. v1 = v0 + e1;  v2 = v0 + e2;  lo.a = min(q0.a, q1.a, q2.a), hi.a = max(q0.a, q1.a, q2.a) per axis a
 *                   2. coordinate axes, on the untranslated coordinates: for each axis a, mn / mx over v0.a, v1.a, v2.a:
 *                        require mn <= hi.a and mx >= lo.a       (step 2 of the box rule with the query triangle's bounds as the box)
 *                   3. f1 = q1 - q0;  f2 = q2 - q0;  p_k = v_k - q0
 *                   4. for an axis a: t_k = dot(a, p_k), s1 = dot(a, f1), s2 = dot(a, f2);
 *                        require min(t_0, t_1, t_2) <= max(0, s1, s2) and max(t_0, t_1, t_2) >= min(0, s1, s2)
 *                      applied to 17 axes:
 *                        the two normals n = cross(e1, e2) and m = cross(f1, f2);
 *                        nine edge pairs cross(g, h), g in (e1, e2 - e1, e2) outer, h in (f1, f2 - f1, f2) inner;
 *                        six in-plane edge normals cross(n, g) for the three g, then cross(m, h) for the three h
 *                      (the in-plane axes decide coplanar pairs, where n, m are parallel and every edge pair is parallel to them).
 *                 The result is the conjunction; the order in which the axes are evaluated does not matter.
 *   Acceptance  : every requirement holds and, with `after`, the triangle index is greater than after[i].
 *   Touching    : is decided by this rounded arithmetic.
 *   Guaranteed  : with finite values, a query vertex that is bit-equal to a record's v0 always accepts that record.  For q0 == v0, p_0 is
 *                 0 and lies in every interval that holds 0.  For q1 == v0, p_0 = fl(v0 - q0) is the very f1, so t_0 and s1 are the same
 *                 bits on every axis; likewise q2 and f2.  Step 2 holds because v0.a lies in [lo.a, hi.a].
 *   Degenerate  : a zero-area query triangle is valid, and a zero-area scene record is tested like any other; both are decided by the rule
 *                 as written, which is complete (separates every disjoint pair in exact arithmetic) only for triangles with area.
 *   Invalid     : a query triangle with a non-finite component of q0, q1, q2, f1 or f2 — zero records and total 0 without traversal,
 *                 counted as a query with no tests.  The pads are ignored.
 *   Order, continuation, errors, state, tuning keys, the max_hits cap and the counters are the box query's, word for word, with
 *   "triangles" for the input and "triangles" for the output in the error texts (device entry: the query triangles 16-byte, the rest
 *   4-byte aligned), and with ray counting on rays = query triangles.  The answer does not depend on the tree, the builder or the
 *   visiting order: it is a function of the leaf records (of the admitted triangles, with a mask table set) alone. */
typedef struct fyprt_triangle { float v0[3]; uint32_t pad0; float v1[3]; uint32_t pad1; float v2[3]; uint32_t pad2; } fyprt_triangle; /* 48 B, 16-B aligned on the device */
/* Host memory, blocking.  `triangles`: count x max_hits scene-triangle indices, query-major.  `stats` as fyprt_overlap_boxes'. */
int fyprt_overlap_triangles(fyprt_context* ctx, const fyprt_triangle* tris, const uint32_t* after /* NULL or count */, uint32_t count,
                            uint32_t max_hits, uint32_t* triangles /* count x max_hits */, uint32_t* hit_counts /* NULL or count */,
                            uint32_t* totals /* NULL or count */, fyprt_frame_stats* stats /* may be NULL */);
/* Device memory of the context's GPU, asynchronous on the context stream (fyprt_stream). */
int fyprt_overlap_triangles_device(fyprt_context* ctx, const void* tris, const void* after, uint32_t count, uint32_t max_hits,
                                   void* triangles, void* hit_counts, void* totals);

/* ------------------------------------------------------------------------------------------------- query filters
 * New (no reference counterpart): per-mesh group masks for the five query families above, so that a query can leave a mesh out (snapping
 * a dragged mesh onto its neighbours, clearance around it, a broad phase against everything else) or look at one mesh alone (picking
 * within the selection).  The meshes are the instances ("Query filters").
 *   The mesh mask table M: one 32-bit word per mesh of the uploaded scene.  The query mask Q: one word per context, 0xFFFFFFFF by default.
 *   The rule: the meshes partition the triangle list (upload and append enforce it); a triangle of mesh m is admitted iff (M[m] & Q) != 0.
 *   With a table set, acceptance in the ten entry points fyprt_trace_rays, fyprt_trace_ray_hits, fyprt_nearest_points,
 *   fyprt_overlap_boxes, fyprt_overlap_triangles and their _device forms gets the extra condition "the triangle is admitted".  Nothing
 *   else changes: keys, order, continuation (`after`), unused records, counts, invalid records and error order are as stated above, and
 *   the box and triangle queries' totals count admitted triangles only.  Each answer is the family's rule applied to the leaf records of the admitted triangles alone.  The
 *   closest-hit query keeps its rule for exact-t ties (the first found in traversal order, among admitted triangles); the list queries stay
 *   independent of the tree.
 *   Not touched: frames of every technique, fyprt_render_rays* (its primary pass and the payloads it returns are unfiltered), the
 *   upscaler's primary rays, every denoiser and every scene edit.  With no table set the kernels launched are the unfiltered ones.
 *   Life of the table: fyprt_upload_scene drops it (filter off) and resets Q to all ones; fyprt_append_meshes extends it with 0xFFFFFFFF
 *   per new mesh; fyprt_remove_meshes takes the removed meshes' entries out and moves the rest down in order (removing every mesh leaves
 *   the filter off, as an upload does); a failed call changes nothing; fyprt_regraft_meshes and the geometry, material and texture edits
 *   leave it alone.  The table is per context, as the scene is.
 *   Device data: 4 bytes per leaf record and 4 bytes per node (the OR of the masks below it: a query never enters a sub-tree it does not
 *   admit — an imported or regrafted mesh is one sub-tree), plus 8 bytes per mesh, built on the context stream by the first filtered
 *   query after the table was set or the tree changed (append, removal, regraft and their rebuild fall-backs; not by vertex, transform,
 *   material or texture edits, refits, or a new Q), counted by fyprt_live_device_bytes, released when the filter is switched off and
 *   on destroy.  The device entries stay asynchronous.  With ray counting on a masked node is no node visit and a masked record no
 *   triangle test.
 * fyprt_set_mesh_query_masks: masks == NULL with mesh_count == 0 switches the filter off (the default).  Errors, in this order:
 * FYPRT_EINVAL for a NULL context; FYPRT_EINVAL for a NULL array with a non-zero count or a non-NULL array with count 0; FYPRT_ESTATE
 * before fyprt_upload_scene; FYPRT_EINVAL for a mesh_count different from the scene's mesh count.  Host-only contexts accept the call
 * (the table is kept, there is nothing to build).  The call waits for the context stream. */
int fyprt_set_mesh_query_masks(fyprt_context* ctx, const uint32_t* masks, uint32_t mesh_count);
/* One mask for all later query calls of the context, in any state of the context, before or after the table.  A plain launch argument: a
 * device-entry call uses the value in effect when it was enqueued.  FYPRT_EINVAL for a NULL context. */
int fyprt_set_query_mask(fyprt_context* ctx, uint32_t query_mask);
/* The filter as it is: *mesh_count = the table's length (0: the filter is off), masks (NULL: only the count is wanted) the table, builds
 * the number of times the device data has been built since the context was created.  Any out-pointer but mesh_count may be NULL.
 * FYPRT_EINVAL for a NULL context or mesh_count. */
int fyprt_get_query_filter(fyprt_context* ctx, uint32_t* masks, uint32_t* mesh_count, uint32_t* query_mask, uint64_t* builds);

/* ================================================================================================= radiance queries
 * New (no reference counterpart): the renderer's sample of techniques 0-6 for the caller's own rays — other camera models, light probes,
 * surface bakes, re-rendering a few pixels ("Radiance queries").  Only an uploaded scene is needed (no resize, no camera).
 *   settings   : a frame's fyprt_settings; technique (0..6), light_bounces, sample_count and sky_color are read, with a frame's uint8
 *                casts; every other field is ignored.
 *   rays       : fyprt_ray records.  [tmin, tmax] applies to the PRIMARY segment only, with the FYPRT_QUERY_CLOSEST acceptance rule; bounce
 *                and shadow rays behave as in a frame.  The direction is used as given (-direction is the view vector at the primary hit,
 *                as the camera direction is in a frame): pass unit vectors.
 *   seed       : ray k uses the random sequence of pixel p_k = pixel_indices ? pixel_indices[k] : first_index + k, seeded p_k x frame_index
 *                as a frame seeds pixel x + y*W with its frame index (frame_index >= 1).
 *   radiance4  : count x float4 = exactly what a frame's epilogue adds to the accumulation for this ray: (rgb, 1), or (0,0,0,0) if any
 *                component is non-finite.  A primary miss inside the interval gives (sky, 1), an emitter hit (emission, 1), a ray that
 *                the batched ray queries call invalid (0,0,0,0) and the miss record, without traversal.  So a W x H frame with frame index f
 *                accumulates exactly accum + radiance4 of its camera rays in row-major order with first_index 0 and frame_index f.
 *   payloads   : NULL, or count x 40 B: the primary record, bit-identical to FYPRT_QUERY_CLOSEST for the same ray and interval.
 * Errors, in this order: FYPRT_EINVAL for a NULL context or settings, a technique outside 0..6 (ReSTIR DI / GI are defined over
 * screen-space neighbours and history, not free rays), frame_index 0, NULL rays / radiance4 with count > 0, and (device entry) rays or
 * radiance4 not 16-byte, payloads not 8-byte or pixel_indices not 4-byte aligned; FYPRT_ESTATE on a host-only context or before
 * fyprt_upload_scene; FYPRT_ENOLIGHT for techniques 5 and 6 without emissive triangles or light tree.  count 0 returns FYPRT_OK and
 * launches nothing.
 * No frame state moves (frame index, accumulation, image, payload, depth, normals, reservoirs, frame timings and counters); a query
 * between the two parts of a ReSTIR frame leaves it undisturbed.  The query has its own path state, ray lists, counters and queue heads,
 * allocated on first use for min(count, FYPRT_RENDER_RAYS_CHUNK) rays and kept; larger batches run in chunks of that many rays, with the
 * same results.  Tuning keys 4, 5, 6, 9, 10 and 15 act on its trace launches as on a frame's path stages (and key 18 on NEE's shadow rays).
 * The caller's rays are not reordered.  For the closest-hit query alone, 8x8-tile-ordered camera rays measured faster than row-major
 * ones; for a whole radiance query of 1080p camera rays, row-major order measured slightly faster. */
#define FYPRT_RENDER_RAYS_CHUNK (1u << 21)   /* rays per internal pass; larger batches are split, results unchanged */
/* Host memory, blocking.  `stats` may be NULL: kernel_ms = the hipEvent time over the call's kernels, launches = their number; with ray
 * counting on, rays / box_tests / tri_tests / hits / node_visits are the totals, counted as a frame counts them, part_*[0] = the same. */
int fyprt_render_rays(fyprt_context* ctx, const fyprt_settings* settings, uint32_t frame_index,
                      const fyprt_ray* rays, const uint32_t* pixel_indices /* may be NULL */, uint32_t first_index, uint32_t count,
                      float* radiance4, void* payloads /* may be NULL: count x 40 B */, fyprt_frame_stats* stats /* may be NULL */);
/* Device memory of the context's GPU, asynchronous on the context stream (fyprt_stream); it never waits on the device. */
int fyprt_render_rays_device(fyprt_context* ctx, const fyprt_settings* settings, uint32_t frame_index,
                             const void* rays, const uint32_t* pixel_indices, uint32_t first_index, uint32_t count,
                             void* radiance4, void* payloads);

/* ================================================================================================= denoiser
 * New (no reference counterpart): an edge-avoiding a-trous wavelet filter over the frame the context rendered last, on the device, guided
 * by what that frame left there — FYPRT_BUF_ACCUM, the frame index it was divided by, and FYPRT_BUF_PAYLOAD (the primary hit of every
 * pixel, written by every technique).  Call it after a frame (Renderer::Render), before presenting ("Denoiser").
 * The contract.  All arithmetic is binary32 without contraction, in the order written; every division is a true division; subnormals are
 * kept; max(a, b) is (a < b) ? b : a.  n = the frame index the last frame was rendered with.  Per pixel p:
 *   c_p = accum_p.rgb / n.   filterable_p: the payload records a hit (objectIndex >= 0) whose material does not emit
 *   (length(emission) > 0 is the frames' own test).  Misses and directly seen emitters pass through and are never a tap.
 *   a_p = the albedo of the primary hit (material colour or re-quantised bilinear texture sample, as the frames shade it);
 *   d_p = max(a_p, 1e-3) per channel with demodulate_albedo, else 1;  e0_p = c_p / d_p.
 *   Iteration k = 0 .. iterations-1: step s = 2^k, sigma_k = sigma_luminance * 2^-k, h = (1/16, 1/4, 3/8, 1/4, 1/16), taps
 *   q = p + s * (dx, dy), dy outer, dx inner, both -2..2 increasing.  A tap outside the image or not filterable is skipped.  Else
 *     w_n = max(0, (n_p.x n_q.x + n_p.y n_q.y) + n_p.z n_q.z), squared normal_power_log2 times;
 *     g = |(n_p.x D.x + n_p.y D.y) + n_p.z D.z|, D = P_q - P_p;  x_z = g / (sigma_plane * t_p), t_p the primary hit distance;
 *     w_z = 1 / (1 + x_z x_z);   L(e) = (0.2126 e.r + 0.7152 e.g) + 0.0722 e.b;  x_l = |L(e_q) - L(e_p)| / sigma_k;
 *     w_l = 1 / (1 + x_l x_l), or 1 when sigma_luminance <= 0;   w = ((w_n w_z) w_l) (h_dy h_dx); the centre tap has w = 3/8 * 3/8;
 *     e_p <- (sum e_q w) / (sum w), both sums sequential in tap order from +0, per channel.
 *   out_p = e_p * d_p (filterable) or c_p;  radiance4 = (out, accum_p.w / n);  rgba8 = the frame epilogue's tonemap / clamp / pack of it.
 *   So iterations = 0 with demodulate_albedo = 0 returns the frame's own image bit for bit.
 * Errors, in this order: FYPRT_EINVAL for a NULL context / params, a parameter out of range or non-finite, (device entry) rgba8 not
 * 4-byte or radiance4 not 16-byte aligned, both outputs NULL; FYPRT_ESTATE on a host-only context, when no complete frame was rendered
 * since the last fyprt_resize, fyprt_upload_scene, fyprt_update_vertices, fyprt_update_transforms or fyprt_update_materials (each of
 * them invalidates the frame for the denoiser: the payload's triangle indices and texture coordinates belong to the scene they were
 * traced in, and its albedo to the materials it was shaded with; textures change with fyprt_upload_scene only), between the two parts of a fyprt_render_part frame, and on a context that does not
 * render every row (a fyprt_set_rows band, fyprt_set_row_stripes, a group or communicator member).  The bands of a group are denoised by fyprt_group_denoise
 * (multi-GPU section); a communicator's are not.
 * No frame state moves: accumulation, image (internal or external), payload, depth, normals, reservoirs, frame index, frame timings and
 * ray counters are untouched, and the frames rendered afterwards are the frames that would have been rendered without the call.  The
 * denoiser's buffers (guide records, albedo, two colour buffers, host staging: 96 B + up to 20 B per pixel) are allocated on the first
 * call and dropped by fyprt_resize. */
typedef struct fyprt_denoise_params {
    uint32_t iterations;         /* 0..8, default 5 */
    float    sigma_luminance;    /* default 4.0; <= 0 switches the luminance term off */
    float    sigma_plane;        /* default 0.01 (of the hit distance); > 0 and finite */
    uint32_t normal_power_log2;  /* 0..7, default 6 (n.n' to the 64th) */
    uint32_t demodulate_albedo;  /* 0 / 1, default 1 */
} fyprt_denoise_params;
int fyprt_denoise_default_params(fyprt_denoise_params* out);
/* Host memory, blocking; width x height uint32 / float4; either output may be NULL.  `stats` may be NULL: kernel_ms = the hipEvent time
 * over the call's kernels, launches = their number, kernel_ms_part[0] = the prepare kernel, [1] = the iterations. */
int fyprt_denoise(fyprt_context* ctx, const fyprt_denoise_params* params, uint32_t* rgba8, float* radiance4, fyprt_frame_stats* stats);
/* Device memory of the context's GPU, asynchronous on the context stream (fyprt_stream); it never waits on the device. */
int fyprt_denoise_device(fyprt_context* ctx, const fyprt_denoise_params* params, void* rgba8, void* radiance4);

/* ================================================================================================= temporal denoiser
 * New (no reference counterpart): the denoiser above with a memory (the SVGF structure; DESIGN.md §4, "Temporal denoiser").  The context
 * keeps a history record per pixel.  A call reprojects every primary hit of the frame rendered last into the frame the previous call
 * denoised, blends the frame's colour and two luminance moments into what it finds there, derives a per-pixel variance, and runs the
 * a-trous iterations with a luminance stopping function scaled by that variance.  For a moving camera that renders one-sample frames
 * (to_accumulate = 0): call it after every frame, before presenting, in place of fyprt_denoise.
 * The contract.  Arithmetic as for fyprt_denoise: binary32 without contraction in the order written, true divisions, a correctly rounded
 * square root, subnormals kept, max(a, b) = (a < b) ? b : a and min(a, b) = (b < a) ? b : a.  n, c_p, filterable_p, a_p, d_p, e0_p, L(.),
 * P_p, n_p, t_p, h, w_n and w_z are fyprt_denoise's, with params->spatial.  L_p = L(e0_p).
 *   1. Camera.  The library keeps M = projection x view (column j = ((A.c0 B.cj.x + A.c1 B.cj.y) + A.c2 B.cj.z) + A.c3 B.cj.w, as it
 *      forms prev_projection x prev_view) of the camera each frame was rendered with, taken when the frame (its first part) is enqueued:
 *      a fyprt_set_camera between the frame and the call changes nothing.  A call reprojects with the M of the frame the previous temporal
 *      call denoised (frames rendered in between without a call do not count).  The caller's prev_* matrices are not used: they belong to
 *      ReSTIR and to the application's own commit point.
 *   2. Reprojection, per filterable pixel when a history exists.  For r in x, y, w:
 *        clip.r = (M.c0.r P.x + M.c1.r P.y) + (M.c2.r P.z + M.c3.r);   history only if clip.w > 0;
 *        sx = ((clip.x / clip.w) 0.5 + 0.5) W,  sy = ((clip.y / clip.w) 0.5 + 0.5) H  (W, H converted to binary32);
 *        history only if -1 <= sx < W and -1 <= sy < H;   x0 = floor(sx), wx = sx - x0, y0 = floor(sy), wy = sy - y0.
 *      Taps q in the order (x0, y0), (x0+1, y0), (x0, y0+1), (x0+1, y0+1) with b = (wx or 1 - wx) * (wy or 1 - wy).  A tap is valid when
 *      it is inside the image, its history record is filterable with N >= 1, b > 0, (n_p.x n_q.x + n_p.y n_q.y) + n_p.z n_q.z >=
 *      normal_min and |(n_p.x D.x + n_p.y D.y) + n_p.z D.z| <= plane_max * t_p, D = P_q - P_p (P_q, n_q of the history record).
 *      Over the valid taps in that order, from +0: sw = sum b, sc = sum colour_q b (per channel), s1 = sum m1_q b, s2 = sum m2_q b;
 *      N_hist = the largest N_q.
 *   3. Integration.  With a valid tap: N = min(N_hist + 1, history_limit);  if N = 1 (history_limit = 1) the new sample alone is taken;
 *      otherwise a = 1 / N, h = s / sw, x = h + (x_new - h) a for the colour channels (x_new = e0_p) and the two moments (x_new = L_p and
 *      L_p L_p).  Without one: N = 1, colour e0_p, moments (L_p, L_p L_p).  A pixel that is not filterable: N = 0, the same colour and
 *      moments, variance 0.
 *   4. Variance.  N >= 4: v = max(0, m2 - m1 m1).  N < 4: over the taps q = p + (dx, dy), dy outer, dx inner, both -2..2 increasing,
 *      inside the image and filterable, with w = w_n w_z:  S0 = 1 + sum w, S1 = L_p + sum L_q w, S2 = L_p L_p + sum (L_q L_q) w (the
 *      centre comes first with weight 1 and is not a tap), M1 = S1 / S0, M2 = S2 / S0, v = max(0, M2 - M1 M1) * (4 / N).
 *   5. Filter.  e = the integrated colour.  Iteration k = 0 .. iterations-1 is fyprt_denoise's (step 2^k, taps, order, w_n, w_z, h)
 *      with: vbar_p = (sum v_q g) / (sum g) over q = p + (dx, dy), dy outer, dx inner, both -1..1, inside the image and filterable (the
 *      centre among them), g = g_dy g_dx, g = (1/4, 1/2, 1/4), both sums from +0;  x_l = |L(e_q) - L(e_p)| / (sigma_luminance *
 *      sqrt(vbar_p) + 1e-4) (w_l = 1 when sigma_luminance <= 0);  and the variance is filtered along: v_p <- (sum v_q (w w)) / ((sum w)
 *      (sum w)), the centre tap first in its place of the tap order with w = 3/8 * 3/8 as for the colour.
 *   6. History written (FYPRT_BUF_TEMPORAL): P_p, t_p | n_p, filterable_p (1.0 / 0.0) | colour, N | m1, m2, the variance of step 4, 0.
 *      The colour is the output of iteration 0 when feedback = 1 and iterations >= 1, else the integrated colour.
 *      Output: out_p = e_p * d_p (filterable) or c_p; radiance4.w and rgba8 as fyprt_denoise forms them.
 *   So the first call after a reset with iterations = 0 and demodulate_albedo = 0 returns the frame's own image bit for bit, and
 *   history_limit = 1 makes every call a first call.
 * The history is dropped — the next call behaves as a first call — by fyprt_resize, fyprt_upload_scene, fyprt_update_vertices,
 * fyprt_update_transforms (world positions of an edited scene are not comparable), fyprt_update_materials (nor are its colours) and
 * fyprt_denoise_temporal_reset.  (fyprt_denoise_temporal_set_motion, below, lets the history live through the two geometry edits.)
 * Errors, in this order: FYPRT_EINVAL for a NULL context / params, history_limit outside 1..256, feedback > 1, normal_min or plane_max
 * not finite, plane_max <= 0; then everything fyprt_denoise refuses, in its order, with params->spatial (its FYPRT_EINVAL cases, then
 * its FYPRT_ESTATE cases).  The bands of a group are denoised by fyprt_group_denoise_temporal (multi-GPU section), whose contract is this
 * one with one more term, the band's history window.
 * No frame state moves, as for fyprt_denoise, and the two denoisers do not disturb each other: the history lives in buffers of its own
 * (two of 64 B and two of 4 B per pixel, allocated on the first temporal call, dropped by fyprt_resize); the guide, albedo and colour
 * buffers of fyprt_denoise are shared scratch, and FYPRT_BUF_ALBEDO is written by either.
 * Static cameras: techniques 0-6 seed a pixel with pixel x frame index, and to_accumulate = 0 holds the frame index at 1, so a static
 * camera then renders the same frame every time (the reference's seeding).  The temporal variance of identical frames is zero, the
 * luminance term shuts and the result degrades towards the unfiltered frame; use a ReSTIR technique (its seeds move on) or accumulate. */
typedef struct fyprt_temporal_params {
    fyprt_denoise_params spatial;   /* iterations, sigma_luminance, sigma_plane, normal_power_log2, demodulate_albedo; defaults as there */
    uint32_t history_limit;         /* 1..256, default 32: the blend factor is never below 1 / history_limit */
    float    normal_min;            /* default 0.9; finite */
    float    plane_max;             /* default 0.02 (of the hit distance); > 0 and finite */
    uint32_t feedback;              /* 0 / 1, default 1 */
} fyprt_temporal_params;
int fyprt_denoise_temporal_default_params(fyprt_temporal_params* out);
/* Host memory, blocking, as fyprt_denoise.  stats: kernel_ms_part[0] = prepare, [1] = reprojection + variance, [2] = the iterations. */
int fyprt_denoise_temporal(fyprt_context* ctx, const fyprt_temporal_params* params, uint32_t* rgba8, float* radiance4, fyprt_frame_stats* stats);
/* Device memory, asynchronous on the context stream, as fyprt_denoise_device. */
int fyprt_denoise_temporal_device(fyprt_context* ctx, const fyprt_temporal_params* params, void* rgba8, void* radiance4);
/* Drops the history: the next temporal call behaves as a first call.  Call it when the scene is replaced by other means than the above
 * or the camera cuts. */
int fyprt_denoise_temporal_reset(fyprt_context* ctx);
/* Object motion, opt-in: enabled = 1 keeps the history through fyprt_update_vertices and fyprt_update_transforms (dragging a mesh while the
 * temporal denoiser runs), enabled = 0 (the default) is everything above unchanged, kernels included.  FYPRT_EINVAL for a NULL context or
 * a value other than 0 / 1.  A call with the value in effect does nothing; a call that changes it drops the history as
 * fyprt_denoise_temporal_reset does and releases the snapshot below.  Allowed on host-only contexts (the flag is stored; the temporal calls
 * stay refused).
 * With 1: the two geometry edits no longer drop the history.  If a history exists and no snapshot is pending, the edit first copies the
 * world vertices (positions and normals) as they are on the device into a per-context snapshot buffer — device to device, on the context
 * stream, after the call's own wait for the context's streams and complete before the edit writes a vertex.  The snapshot is pending from that
 * copy until the next successful temporal call, which consumes it; further edits before that call leave it alone, frames rendered in
 * between without a temporal call do not matter, so the snapshot is always the geometry of the frame the previous temporal call
 * denoised.  fyprt_upload_scene, fyprt_update_materials, fyprt_resize, fyprt_denoise_temporal_reset and a change of the mode drop
 * history and snapshot; a refused temporal call drops neither.
 * The edits still invalidate the frame for both denoisers: render one before the next call.  The snapshot buffer (32 B per vertex and a
 * byte per triangle) is allocated at the first snapshot and released by fyprt_upload_scene and by switching the mode off; a context that
 * never switches the mode on allocates nothing.
 * The contract: step 2 above when a snapshot is pending.  Arithmetic as everywhere in it; dot(x, y) = (x.x y.x + x.y y.y) + x.z y.z; no
 * special cases (a comparison with a NaN is false).  For a filterable pixel p whose payload names triangle T: (a, b, c) = T's current world
 * positions, (a', b', c') and (na', nb', nc') = T's positions and normals in the snapshot.  T is moved when any of the 18 position and
 * normal floats of its three vertices differs bit-wise between snapshot and current.
 *   T not moved: P' = P_p, n' = n_p — the pixel goes through the arithmetic above exactly.
 *   T moved:     e1 = b - a, e2 = c - a, d = P_p - a;  d11 = dot(e1, e1), d12 = dot(e1, e2), d22 = dot(e2, e2), p1 = dot(d, e1),
 *                p2 = dot(d, e2);  det = d11 d22 - d12 d12;  beta = (d22 p1 - d12 p2) / det, gamma = (d11 p2 - d12 p1) / det,
 *                alpha = (1 - beta) - gamma;  P' = (a' alpha + b' beta) + c' gamma and m = (na' alpha + nb' beta) + nc' gamma per
 *                component;  n' = m (1 / sqrt(dot(m, m))) (two roundings).
 *   Step 2 with P', n': clip is formed from P'; a tap is valid when dot(n', n_q) >= normal_min and |dot(n', P_q - P')| <= plane_max t_p;
 *   everything else of step 2 and steps 3 to 6 are unchanged — the history record written still holds the current P_p, n_p.  A degenerate
 *   triangle gives a non-finite P' or n' and, through the comparisons, no history (N = 1) or an invalid tap.
 * This is SVGF's motion vector, from the two vertex sets instead of a rasteriser.  The limit: a long history of a surface whose lighting
 * changes as it moves lags behind it (fast drags look worse with the history kept than without); history_limit is the
 * control.  ReSTIR's own temporal reuse is not touched. */
int fyprt_denoise_temporal_set_motion(fyprt_context* ctx, int enabled);

/* ================================================================================================= upscaler
 * New (no reference counterpart): denoise at the rendered size W x H, present at sW x sH, s = 2, 3 or 4 ("Upscaler").  The
 * call runs the low-res stage of either denoiser, traces primary rays only at sW x sH, interpolates the demodulated colour under the
 * hi-res guide records and multiplies by the hi-res albedo: geometric edges and texture detail arrive at the presented size, lighting at
 * the rendered one.  Camera::RecalculateRayDirections forms (float)x / (float)width, and (float)(s x) / (float)(s W) is the correctly
 * rounded value of the same rational: hi-res pixel (s x, s y) has bit for bit the ray of low-res pixel (x, y), so the rendered samples sit
 * exactly on every s-th hi-res pixel.
 * The contract.  Arithmetic as for fyprt_denoise.  W, H, n, c_p, filterable_p, a_p, d_p, P_p, n_p, t_p, w_n and w_z are fyprt_denoise's,
 * with params->filter.spatial.  Capital letters name hi-res pixels Q = (X, Y), X < sW, Y < sH.
 *   1. Low-res stage.  temporal = 0: fyprt_denoise up to its last iteration.  temporal = 1: steps 1 to 6 of fyprt_denoise_temporal with
 *      params->filter — the history record, the consumed motion snapshot and FYPRT_BUF_TEMPORAL are exactly what that call would leave.
 *      e_p = the colour after the last iteration (iterations = 0: e0_p, or the integrated colour; never the feedback colour).
 *      out_p = e_p * d_p (filterable) or c_p: the pixel either denoiser would have output.
 *   2. Hi-res guides.  The primary ray of Q is Camera::RecalculateRayDirections for a viewport sW x sH with the inverse matrices and the
 *      position of the camera the frame was enqueued with (taken where the temporal denoiser's M is taken: a fyprt_set_camera between
 *      frame and call changes nothing).  The primary record of Q is, bit for bit, the FYPRT_BUF_PAYLOAD record a context resized to
 *      sW x sH with that camera and scene writes; hence the record of (s x, s y) is the low-res pixel's.  filterable_Q, a_Q, d_Q, P_Q, n_Q,
 *      t_Q are derived from it as fyprt_denoise derives them.  Pass-through colour of a Q that is not filterable: a miss takes the sky
 *      colour of the settings the frame was rendered with (taken with the camera), a directly seen emitter the material's emission as the
 *      frames form it (emission_color * emission_power).
 *   3. Resolve.  x0 = X div s, y0 = Y div s, fx = X - s x0, fy = Y - s y0.
 *      Aligned (fx = fy = 0): out_Q = out_(x0, y0), no arithmetic.   Not aligned, Q not filterable: out_Q = the pass-through colour.
 *      Not aligned, Q filterable: tx = (float)fx / (float)s, ty likewise; taps q = (x0 + dx, y0 + dy), dy outer, dx inner, both 0..1;
 *        b = (dx ? tx : 1 - tx) * (dy ? ty : 1 - ty).  A tap is usable when it is inside the W x H image, filterable_q holds and b > 0.
 *        w_n = max(0, dot(n_Q, n_q)) squared normal_power_log2 times;  x_z = |dot(n_Q, P_q - P_Q)| / (sigma_plane * t_Q),
 *        w_z = 1 / (1 + x_z x_z);  w = (w_n w_z) b   (dot(a, b) = (a.x b.x + a.y b.y) + a.z b.z).
 *        Over the usable taps in order, from +0: S = sum w, C = sum e_q w, B = sum b, D = sum e_q b (per channel).
 *        E_Q = C / S if S > 0; otherwise E_Q = D / B if a usable tap exists; otherwise out_Q = out_(x0, y0).
 *        With an E_Q: out_Q = E_Q * d_Q (d_Q = 1 without demodulate_albedo).
 *      radiance4 = (out_Q, accum_(x0, y0).w / n);  rgba8 = the frame epilogue's tonemap / clamp / pack of it.
 *      There is no luminance term: no hi-res colour exists to compare.
 *   So out[::s, ::s] of a call is, bit for bit, the output of fyprt_denoise / fyprt_denoise_temporal with the same parameters.
 * Errors, in this order: FYPRT_EINVAL for a NULL context / params, scale outside 2..4 or temporal > 1, with temporal = 1 the parameter
 * cases of fyprt_denoise_temporal (with 0 only filter.spatial is read), sW * sH beyond what fyprt_resize accepts, then everything
 * fyprt_denoise refuses with FYPRT_EINVAL (parameter, alignment, both outputs NULL); then its FYPRT_ESTATE cases in its order (host-only
 * context, no complete frame, between the two parts of a frame, bands / stripes / group and communicator members).
 * No frame state moves.  With temporal = 0 the temporal history is untouched; with 1 the call IS a temporal call.  FYPRT_BUF_ALBEDO is
 * written as by either denoiser.  Afterwards FYPRT_BUF_UPSCALE_GUIDE and FYPRT_BUF_UPSCALE_ALBEDO hold the hi-res records of step 2.  The
 * hi-res buffers (48 B per hi-res pixel, plus up to 20 B of host-entry staging) are allocated on the first call, reallocated when scale
 * changes (that call first waits for the context stream: an earlier call may still write the old ones) and dropped by fyprt_resize and
 * fyprt_destroy. */
typedef struct fyprt_upscale_params {
    uint32_t scale;                 /* 2..4, default 2: the output is scale*W x scale*H */
    uint32_t temporal;              /* 0 (default): the low-res stage is fyprt_denoise with filter.spatial;
                                       1: it is fyprt_denoise_temporal with filter, and the call IS a temporal call */
    fyprt_temporal_params filter;   /* defaults of fyprt_denoise_temporal_default_params */
} fyprt_upscale_params;
int fyprt_upscale_default_params(fyprt_upscale_params* out);
/* Host memory, blocking; scale*width x scale*height uint32 / float4; either output may be NULL.  `stats` may be NULL: kernel_ms_part[0] =
 * the low-res stage (prepare through the last iteration), [1] = the hi-res primary kernel, [2] = the resolve kernel, launches = their number. */
int fyprt_denoise_upscale(fyprt_context* ctx, const fyprt_upscale_params* params, uint32_t* rgba8, float* radiance4, fyprt_frame_stats* stats);
/* Device memory of the context's GPU, asynchronous on the context stream, as fyprt_denoise_device. */
int fyprt_denoise_upscale_device(fyprt_context* ctx, const fyprt_upscale_params* params, void* rgba8, void* radiance4);

/* ================================================================================================= multi-GPU
 * The reference renders on one GPU (Renderer.cu:13-284); there is no reference interface for this section.  It splits ONE
 * Renderer::Render call over several GPUs by image rows: every GPU holds the whole scene and renders a band;
 * reservoirs, G-buffers and accumulation stay on the GPU that owns the rows; the RGBA8 bands are gathered once per frame.
 * `row_bounds` always has (number of bands + 1) entries: band k = rows [row_bounds[k], row_bounds[k+1]), row_bounds[0] = 0,
 * the last entry = height.
 * Halo mode (the `radius` rows either side of a band that ReSTIR Part 2's spatial reuse reads):
 *   0 recompute: every band also runs Part 1 on its halo rows; frame 1 equals the single-GPU frame, later frames differ (unbiased)
 *                near band borders because the halo rows have no temporal history;
 *   1 exchange : the bands send each other the Part-1 records (and the temporal history) of those rows — a static-camera
 *                sequence then equals the single-GPU sequence bit for bit on every frame, and Part 1 does no duplicate work
 *                (shown for the peer-copy transport fyprt_group_*; the RCCL transport fyprt_comm_* runs the same plan but has only
 *                executed with a one-rank communicator so far: INTEGRATION.md, "Verification status"). */
typedef struct fyprt_group fyprt_group;
/* --- one process, one context per GPU (a C++ host such as the reference's MainLayer): peer copies, no collective library */
int fyprt_group_create(fyprt_context** contexts, int n, const uint32_t* row_bounds, fyprt_group** out);
void fyprt_group_destroy(fyprt_group* group);                       /* the contexts stay alive */
int fyprt_group_set_rows(fyprt_group* group, const uint32_t* row_bounds);
int fyprt_group_set_halo_mode(fyprt_group* group, int mode);
/* stripe_rows > 0: frames of the per-pixel techniques are split into interleaved stripes (fyprt_set_row_stripes, context i = part i),
 * ReSTIR frames keep the row bands; the gather moves stripes instead of bands.  The rows a context accumulates are the rows it
 * renders: restart the accumulation (fyprt_reset_frame_index on every context) when changing this setting, and — while it is on —
 * when switching between a ReSTIR and a per-pixel technique (the reference's host restarts it on any change of settings anyway). */
int fyprt_group_set_interleave(fyprt_group* group, uint32_t stripe_rows);
int fyprt_group_render(fyprt_group* group, const fyprt_settings* settings);   /* one frame on every band; asynchronous */
int fyprt_group_gather(fyprt_group* group, int root);               /* all bands' RGBA8 rows into context `root`'s image; asynchronous */
int fyprt_group_synchronize(fyprt_group* group);
/* fyprt_denoise for the frame the group rendered last: every context filters its own band, the bands pull the rows either side that
 * their taps reach from the contexts that own them, and the output rows are collected on one context.  The outputs are, bit for bit,
 * what fyprt_denoise with the same parameters returns for a single context holding the same frame: the bands' accumulation and payload
 * rows stitched together, and the same frame index.
 * Errors, in this order: FYPRT_EINVAL for a NULL group / params, every parameter case of fyprt_denoise, `root` out of range, (device
 * entry) misaligned outputs, both outputs NULL; FYPRT_ESTATE for a member without a complete frame (fyprt_denoise's conditions),
 * members whose last frames differ in frame index, a last group frame that was striped (fyprt_group_set_interleave), a member whose
 * rows are not its band of the group (fyprt_set_rows behind the group).  The message is the offending member's.
 * No frame state moves on any member.  Afterwards FYPRT_BUF_ALBEDO is valid on every member for its own rows.  The buffers (those of
 * fyprt_denoise, the staging being the band's rows) are allocated per member on first use and dropped by fyprt_resize.
 * fyprt_denoise* on a group member stays refused. */
/* Host memory, blocking; width x height uint32 / float4 of the WHOLE frame; either output may be NULL.  band_ms: NULL or one float per
 * band, the hipEvent time from its first to its last enqueued operation on its own stream (waits for its neighbours included). */
int fyprt_group_denoise(fyprt_group* group, const fyprt_denoise_params* params, uint32_t* rgba8, float* radiance4, float* band_ms);
/* Device memory on context `root`'s GPU, asynchronous: complete on root's stream (fyprt_stream of that context); no host wait. */
int fyprt_group_denoise_device(fyprt_group* group, const fyprt_denoise_params* params, int root, void* rgba8, void* radiance4);
/* fyprt_denoise_temporal for the frames the group renders: every context keeps the history of its own rows, reprojects and filters its
 * band, and pulls what its kernels read beyond the band from the rows' owners.  A history tap may lie anywhere the camera motion points,
 * so the rows of history a band can see are bounded, and the bound is part of the contract.
 * The contract.  Band k owns the rows [b, e); R = min(history_rows, height); its HISTORY WINDOW is the rows [max(0, b - R), min(height,
 * e + R)).  The output rows and the history records of band k are fyprt_denoise_temporal's contract, steps 1 to 6, evaluated on the
 * stitched frame (every band's accumulation, payload and history rows taken from their owners, the same frame index n), with one
 * addition in step 2: a tap q of a pixel p is valid only if its row also lies inside the history window of the band that owns p.  For
 * its own pixels the band sees a history in which every record outside its window is not filterable.  Nothing else changes: the 5 x 5
 * estimate of step 4, the 3 x 3 variance prefilter and the a-trous taps of step 5 read the real neighbours across band borders — a
 * neighbour in another band enters them as its owner computed it, under that band's window.
 *   So: if every otherwise valid tap of every pixel lies inside its band's window, the outputs and the stitched FYPRT_BUF_TEMPORAL are, bit
 *   for bit, those of fyprt_denoise_temporal on a single context running the same sequence; history_rows >= height guarantees it
 *   unconditionally.  A pixel whose reprojection leaves the window starts over with N = 1, as a disocclusion does; history_rows is the
 *   control.  FYPRT_GROUP_HISTORY_ROWS is derived, not measured: at 64 B per pixel, 32 rows are the bytes the spatial call already pulls
 *   per band side at its default 5 iterations (32 rows of 32 B guide records + 62 rows of 16 B colour: 3.9 MB at 1080p), so the temporal
 *   call at most doubles the traffic per side.
 * Whose history.  The history belongs to the group.  A call finds one only if every member holds a history written by this group's
 * previous successful temporal call (or moved by fyprt_group_set_rows since) and all members keep the same projection x view, bit for
 * bit, for the frame that call denoised.  Otherwise the call is a first call on every member: whatever drops one member's history
 * (fyprt_resize, fyprt_upload_scene, the edits, fyprt_denoise_temporal_reset, a change of the motion mode) or replaces it (a
 * single-context temporal call before the context joined the group) makes the next group call a first call for the whole group.
 * fyprt_group_denoise_temporal_reset drops every member's history.  After a call FYPRT_BUF_TEMPORAL is valid on every member for its
 * own rows, FYPRT_BUF_ALBEDO as after fyprt_group_denoise.  fyprt_denoise_temporal* on a group member stays refused.
 * Rows that change owner.  While the group holds a history, fyprt_group_set_rows also moves the 64-byte history records of the rows
 * that change owner, from the old owner's current history buffer into the new owner's, beside the accumulation and the ReSTIR records.
 * With history_rows >= height a sequence with moving borders therefore stays the single-context sequence.  A group without a temporal
 * history moves exactly what it moved before.
 * Object motion.  fyprt_denoise_temporal_set_motion stays per context (and so does the scene: the caller applies every edit to every
 * member).  A group call requires every member in the same mode and the same snapshot state (pending or not).  With a snapshot pending
 * every band runs the motion form on its rows, and every member consumes its snapshot.
 * Errors, in this order: FYPRT_EINVAL for a NULL group / params; fyprt_denoise_temporal's parameter cases (its own, then the spatial
 * part's); fyprt_group_denoise's remaining FYPRT_EINVAL cases (root, alignment, both outputs NULL); FYPRT_ESTATE for
 * fyprt_group_denoise's state cases in its order; for members whose last frames differ in camera matrix; for members that differ in
 * motion mode or snapshot state.  The message is the offending member's.  A refused call drops nothing.
 * Outputs, root, band_ms, alignment and "no frame state moves on any member" are exactly fyprt_group_denoise's.  The history and
 * variance buffers are those of fyprt_denoise_temporal, full-size per member.
 * Out of scope: an RCCL transport (fyprt_comm_*), striped frames (refused, as by fyprt_group_denoise), and a window that sizes itself
 * from the camera motion (it would need a host wait). */
#define FYPRT_GROUP_HISTORY_ROWS 32u
int fyprt_group_denoise_temporal(fyprt_group* group, const fyprt_temporal_params* params, uint32_t history_rows, uint32_t* rgba8, float* radiance4, float* band_ms);
int fyprt_group_denoise_temporal_device(fyprt_group* group, const fyprt_temporal_params* params, uint32_t history_rows, int root, void* rgba8, void* radiance4);
int fyprt_group_denoise_temporal_reset(fyprt_group* group);
/* fyprt_denoise_upscale for the frame the group rendered last: every context runs the low-res stage on its band, traces the hi-res primary
 * rays of its own hi-res rows and resolves them; the hi-res output rows are collected on one context.
 * The contract is fyprt_denoise_upscale's, steps 1 to 3, evaluated on the stitched frame, with the low-res stage replaced by the group's:
 *   temporal = 0: fyprt_group_denoise up to its last iteration.
 *   temporal = 1: steps 1 to 6 of fyprt_group_denoise_temporal with params->filter and `history_rows` (read only in this mode), history
 *     window included, and the call IS a group temporal call: the group's history is found or not found as that call finds it, written
 *     as it writes it, moved by fyprt_group_set_rows as before, and the motion snapshot is consumed on every member.
 * Band k = the low-res rows [b, e) owns the hi-res rows [s b, s e).  It traces their primary rays itself (step 2) with its own copy of the
 * camera and sky colour the frame was enqueued with, and resolves them itself (step 3).  The resolve of hi-res row Y reads the low-res
 * rows y0 = Y div s and y0 + 1; for the last s - 1 hi-res rows of a band y0 + 1 = e belongs to the next band, and that row's guide record
 * and its colour e after the last iteration come from its owner.  Row `height` is outside the image, as in the single call.
 *   So: with temporal = 0 the outputs are, bit for bit, fyprt_denoise_upscale's for a single context holding the same frame; with
 *   temporal = 1 the same holds wherever fyprt_group_denoise_temporal equals the single context — always with history_rows >= height.
 *   out[::s, ::s] is the output of the matching group denoiser call.
 * Afterwards FYPRT_BUF_UPSCALE_GUIDE and FYPRT_BUF_UPSCALE_ALBEDO are valid on every member for its own hi-res rows, as FYPRT_BUF_ALBEDO
 * is after fyprt_group_denoise; FYPRT_BUF_ALBEDO and FYPRT_BUF_TEMPORAL are left as after the matching group denoiser call.  No frame
 * state moves on any member.  fyprt_denoise_upscale* on a group member stays refused.
 * Errors, in this order: FYPRT_EINVAL for a NULL group / params; fyprt_denoise_upscale's parameter cases in its order (scale / temporal
 * out of range, with temporal = 1 the temporal parameter cases, the hi-res size limit, the spatial parameter cases); fyprt_group_denoise's
 * remaining FYPRT_EINVAL cases (root, alignment of the hi-res outputs on root's context, both outputs NULL); FYPRT_ESTATE for
 * fyprt_group_denoise's state cases in its order; for members whose last frames differ bit-wise in camera (inverse projection, inverse
 * view, position) or sky colour — the bands would trace different hi-res frames; with temporal = 1 fyprt_group_denoise_temporal's
 * camera-matrix and motion-mode cases.  The message is the offending member's.  A refused call drops nothing and allocates nothing.
 * Memory: the hi-res guide and albedo buffers are FULL SIZE on every member (48 B per hi-res pixel: 400 MB per member at 3840 x 2160), as
 * every other group buffer and as fyprt_read_buffer expects; the staging is the band's hi-res rows.  They are allocated on the first call,
 * reallocated when scale changes (that call first waits for the member's stream and for the earlier root's collect), dropped by
 * fyprt_resize and counted by fyprt_live_device_bytes.  Band-sized hi-res buffers are out of scope, as are an RCCL transport and striped
 * frames.
 * Outputs: scale*width x scale*height uint32 / float4 of the WHOLE frame; root, band_ms, alignment and "either output may be NULL, not
 * both" are exactly fyprt_group_denoise's. */
int fyprt_group_denoise_upscale(fyprt_group* group, const fyprt_upscale_params* params, uint32_t history_rows, uint32_t* rgba8, float* radiance4, float* band_ms);
int fyprt_group_denoise_upscale_device(fyprt_group* group, const fyprt_upscale_params* params, uint32_t history_rows, int root, void* rgba8, void* radiance4);
/* --- one process per GPU: RCCL over xGMI (librccl.so.1 is opened on first use).  Rank 0 calls fyprt_comm_unique_id and hands
 *     the 128 bytes to the other ranks (any transport); every rank then calls fyprt_comm_init_rank on its resized context. */
int fyprt_comm_unique_id(void* id128);
int fyprt_comm_init_rank(fyprt_context* ctx, int world_size, int rank, const void* id128, const uint32_t* row_bounds);
int fyprt_comm_set_rows(fyprt_context* ctx, const uint32_t* row_bounds);
int fyprt_comm_set_halo_mode(fyprt_context* ctx, int mode);
int fyprt_comm_set_interleave(fyprt_context* ctx, uint32_t stripe_rows);       /* as fyprt_group_set_interleave; same value on every rank */
int fyprt_comm_render(fyprt_context* ctx, const fyprt_settings* settings);    /* this rank's band; collective (every rank calls it); asynchronous */
int fyprt_comm_gather(fyprt_context* ctx, int root /* < 0: every rank gets the frame */);   /* grouped ncclBroadcast per band, in place */
void fyprt_comm_destroy(fyprt_context* ctx);
/* --- building blocks */
/* The two parts of a ReSTIR frame as separate asynchronous calls, for a host with its own transport for the halo rows. */
int fyprt_render_part(fyprt_context* ctx, const fyprt_settings* settings, int part /* 1 or 2 */);
/* Cost-balanced bands: new boundaries from the milliseconds each band took (fyprt_last_frame_ms), at most `max_shift` rows per
 * boundary and call, bands at least `min_rows` high.  Pure arithmetic: the rows change owner with fyprt_group_set_rows /
 * fyprt_comm_set_rows, which move their accumulation and temporal history along. */
int fyprt_balance_rows(const uint32_t* row_bounds, const float* band_ms, int n, uint32_t min_rows, uint32_t max_shift, uint32_t* new_bounds);
int fyprt_last_frame_ms(fyprt_context* ctx, float* ms);
/* The transfers of one halo exchange: (receiver, owner, first row, end row) per entry; returns the number of entries. */
int fyprt_halo_plan(const uint32_t* row_bounds, int n, uint32_t halo, uint32_t height, int wrap_row, uint32_t* out4, int capacity);
/* The transfers of one fyprt_group_denoise* call in issue order: (stage, receiver, owner, first row, end row) per entry.  Stage 0: the
 * guide records (32 B per pixel), 2^iterations rows either side of the band; stage 1 + k: the colour buffer iteration k reads (16 B per
 * pixel), 2^(k+1) rows; clipped to the image.  Pure host arithmetic.  Returns the number of entries (also when `capacity` is smaller;
 * nothing is written beyond it), FYPRT_EINVAL for a bad table or iterations > 8. */
int fyprt_group_denoise_plan(const uint32_t* row_bounds, int n, uint32_t height, uint32_t iterations, uint32_t* out5, int capacity);
/* The transfers of one fyprt_group_denoise_temporal* call in issue order, entries as above, sized by what each kernel reads.  Stage 0:
 * the guide records (32 B), max(2, 2^iterations) rows — the 5 x 5 estimate of step 4 reads 2 rows even without an iteration; stage 1: the
 * prepared colour e0 | L (16 B), 2 rows (step 4's L_q); stage 2: the history (64 B), min(history_rows, height) rows — listed for the
 * history_rows given, a call without a history skips it; stage 3 + k: the colour (16 B) and the variance (4 B) iteration k reads,
 * 2^(k+1) rows.  Pure host arithmetic; returns and errors as fyprt_group_denoise_plan. */
int fyprt_group_denoise_temporal_plan(const uint32_t* row_bounds, int n, uint32_t height, uint32_t iterations, uint32_t history_rows, uint32_t* out5, int capacity);
/* The transfers of one fyprt_group_denoise_upscale* call in issue order, entries as above: the plan of the low-res stage
 * (fyprt_group_denoise_plan, or with temporal != 0 fyprt_group_denoise_temporal_plan for `history_rows`), then one more stage, numbered
 * 1 + iterations (spatial) or 3 + iterations (temporal): for every band k but the last one entry (k, owner of row e_k, e_k, e_k + 1) — the
 * colour buffer that holds e after the last iteration (16 B per pixel), the low-res row the band's last hi-res rows tap.  The row's guide
 * record needs no entry: stage 0 already brings at least one guide row below the band (2^iterations >= 1 rows; temporal max(2, ...)).
 * The spatial plan without an iteration has no stage 0, and the call then moves the guide record with the colour (48 B per pixel).  Pure
 * host arithmetic; returns and errors as fyprt_group_denoise_plan. */
int fyprt_group_denoise_upscale_plan(const uint32_t* row_bounds, int n, uint32_t height, uint32_t iterations, uint32_t temporal, uint32_t history_rows,
                                     uint32_t* out5, int capacity);
/* The point-to-point operations rank `rank` issues inside ONE RCCL group section, in issue order — kind 0: a halo exchange over
 * `row_bounds`; kind 1: fyprt_comm_set_rows from `row_bounds` to `new_bounds`.  (is_recv, peer, buffer, byte offset, bytes) per
 * operation; returns their number.  Pure host arithmetic (no device, no RCCL): lets a test check that the two ends of every pair of
 * ranks list the same byte counts in the same order, which is what RCCL's matching needs. */
int fyprt_comm_ops(int kind, const uint32_t* row_bounds, const uint32_t* new_bounds, int n, uint32_t halo, uint32_t height, int wrap_row, uint32_t width,
                   int rank, const uint32_t* bytes_per_pixel, int nbuf, uint64_t* out5, int capacity);

/* Library / build identification ("fyprt <version> gfx950 ..."). */
const char* fyprt_version(void);

/* Bytes of device memory the library's buffers hold right now, over every context of the process: it returns to its earlier value
 * once everything created since has been destroyed. */
uint64_t fyprt_live_device_bytes(void);

#ifdef __cplusplus
}
#endif
#endif /* FYPRT_H */
