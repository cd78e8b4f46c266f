// C++ host facade over the C ABI (include/fyprt.h) with the public surface of the reference's
// `Renderer` (FYPRayTracer/src/Classes/Core/Renderer.h:41-56), so the call sites in
// MainLayer::Render (WalnutApp.cpp:878-910) and SceneManager (SceneManager.cpp:14,65,81) keep
// their shape:  OnResize / Render(scene, camera) / ResetFrameIndex / GetSettings /
// GetCurrentFrameIndex / GetRenderImageDataPtr / Resize*Buffers / FreeDynamicallyAllocatedMemory /
// SetSceneToBeUpdatedFlag.  `GetFinalRenderImage()` (a Walnut::Image, i.e. a Vulkan upload) becomes
// an optional presenter callback — Walnut/Vulkan is outside this path.
//
// Templated on the caller's Scene / Camera types: anything exposing the reference's member names
// (`worldVertices`, `triangles`, `materials`, `meshes[i].{indexStart,indexCount,materialIndex}`,
// `textures[i].{pixels,width,height}`; camera getters `GetProjection()` ... `GetPosition()`,
// `GetViewportWidth/Height()`) works — the reference's own classes do, and so do the glm-free
// stand-ins in HostTypes.h used by the headless harness.
#pragma once
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <functional>
#include <vector>
#include "../../include/fyprt.h"

namespace fyprt_host {

// RenderingSettings.h:5-22, same field names / defaults; layout-compatible with fyprt_settings.
enum SamplingTechniqueEnum { BRUTE_FORCE, UNIFORM_SAMPLING, COSINE_WEIGHTED_SAMPLING, GGX_SAMPLING, BRDF_SAMPLING,
                             LIGHT_SOURCE_SAMPLING, NEE, RESTIR_DI, RESTIR_GI, SamplingTechniqueEnum_COUNT };
struct RenderingSettings {
    bool toAccumulate = true; int lightBounces = 1; int sampleCount = 1; float skyColor[3] = {1, 1, 1};
    SamplingTechniqueEnum currentSamplingTechnique = BRUTE_FORCE; int lightCandidateCount = 4; uint32_t randSeed = 1;
    bool useTemporalReuse = false; bool useSpatialReuse = false; int temporalHistoryLimit = 2; int spatialNeighborNum = 5; int spatialNeighborRadius = 30;
};
static_assert(sizeof(RenderingSettings) == sizeof(fyprt_settings), "RenderingSettings must stay 52 bytes");

class Renderer {
public:
    explicit Renderer(int device = 0) { report(fyprt_create(device, &m_Ctx), "fyprt_create"); }
    ~Renderer() { FreeDynamicallyAllocatedMemory(); }
    Renderer(const Renderer&) = delete;
    Renderer& operator=(const Renderer&) = delete;

    void OnResize(uint32_t width, uint32_t height) {                       // Renderer.cpp:5-41
        if (width == m_Width && height == m_Height) return;
        if (report(fyprt_resize(m_Ctx, width, height), "fyprt_resize")) return;
        m_Width = width; m_Height = height;
        m_RenderImageData.assign((size_t)width * height, 0u);
        m_AccumulationData.assign((size_t)width * height * 4, 0.0f);
    }

    template <class SceneT, class CameraT> void Render(SceneT& scene, CameraT& camera) {   // Renderer.cu:13-284
        if (isSceneUpdated) {                                                                 // :61-69
            // The scene's signature has two parts.  Structure (counts, triangle vertex indices, mesh ranges, texture identities): a change
            // means a full upload, unless only tails grew (an import, below).  Materials (table, per-triangle and per-mesh material index,
            // emissive list): a change alone is applied on the device by fyprt_update_materials, and the acceleration structure is not touched.
            const uint64_t ssig = StructureSignature(scene, CountsOf(scene)), msig = MaterialSignature(scene);
            bool done = false;
            // an import — "Import Mesh" / "Import Texture" (WalnutApp.cpp:668-693, :739-754) only push onto the end of the scene's arrays: when
            // the structure the library holds is unchanged and only tails grew, the tails go to fyprt_append_textures / fyprt_append_meshes.
            // The material part always differs then (new triangles, a longer emissive list): the material path below follows.
            bool appended = false;
            if (m_HaveScene && ssig != m_StructureSig && m_PendingTransforms.empty() && !m_OtherEdits && AppendTails(scene)) { m_StructureSig = ssig; ++m_Appends; appended = true; }
            if (m_HaveScene && ssig == m_StructureSig) {
                // geometry — (a) nothing but mesh transforms moved vertices and the SceneManager told us which (NoteMeshTransform): 64 bytes
                // per mesh go to the device, which recomputes the world vertices itself;  (b) an edit we know nothing about, or the flag
                // alone: every world vertex is uploaded, refit on the device;  (c) a material edit alone moves no vertex
                bool ok = true;
                if (!appended && !m_PendingTransforms.empty() && !m_OtherEdits) {
                    ok = fyprt_update_transforms(m_Ctx, m_PendingMeshes.data(), m_PendingTransforms.data(), (uint32_t)m_PendingMeshes.size()) == FYPRT_OK;
                    if (ok) { ++m_Refits; ++m_TransformUpdates; }
                }
                if (!appended && (m_OtherEdits || !ok || (m_PendingTransforms.empty() && !m_MaterialEdits))) {
                    ok = fyprt_update_vertices(m_Ctx, reinterpret_cast<const fyprt_vertex*>(scene.worldVertices.data()), (uint32_t)scene.worldVertices.size()) == FYPRT_OK;
                    if (ok) ++m_Refits;
                }
                // materials — after the geometry, so that a tick with both edits does fyprt_update_transforms, then fyprt_update_materials
                if (ok && msig != m_MaterialSig) {
                    ok = UpdateMaterials(scene);
                    if (ok) { m_MaterialSig = msig; ++m_MaterialUpdates; }
                }
                done = ok;
            }
            if (!done) {
                if (UploadScene(scene)) {                    // remember the signature only of a scene the library really holds
                    m_StructureSig = ssig; m_MaterialSig = msig; m_HaveScene = true; ++m_Uploads;
                    KeepMaterialIndices(scene); m_Counts = CountsOf(scene);
                } else {
                    m_HaveScene = false;
                }
            }
            isSceneUpdated = false; m_PendingMeshes.clear(); m_PendingTransforms.clear(); m_OtherEdits = false; m_MaterialEdits = false;
        }
        fyprt_camera_desc c{};                                                                // :70 CameraToGPU
        std::memcpy(c.projection, &camera.GetProjection(), 64); std::memcpy(c.view, &camera.GetView(), 64);
        std::memcpy(c.prev_projection, &camera.GetPrevProjection(), 64); std::memcpy(c.prev_view, &camera.GetPrevView(), 64);
        std::memcpy(c.inverse_projection, &camera.GetInverseProjection(), 64); std::memcpy(c.inverse_view, &camera.GetInverseView(), 64);
        std::memcpy(c.position, &camera.GetPosition(), 12);
        c.viewport_width = camera.GetViewportWidth(); c.viewport_height = camera.GetViewportHeight();
        if (report(fyprt_set_camera(m_Ctx, &c), "fyprt_set_camera")) return;
        fyprt_settings s; std::memcpy(&s, &m_Settings, sizeof s);
        if (report(fyprt_render(m_Ctx, &s, &m_LastStats), "fyprt_render")) return;           // :87-237
        report(fyprt_readback(m_Ctx, m_RenderImageData.data(), m_AccumulationData.data()), "fyprt_readback");   // :244-250
        if (m_Present) m_Present(m_RenderImageData.data(), m_Width, m_Height);                // :256 SetData
    }

    // New (no reference counterpart): the edge-avoiding denoiser over the frame Render() just produced (fyprt_denoise; nullptr = the
    // library's defaults) into `rgba8` (width x height ABGR8) — call it after Render, before presenting.  No renderer state moves.
    bool Denoise(const fyprt_denoise_params* params, uint32_t* rgba8) {
        fyprt_denoise_params p;
        if (params) p = *params; else fyprt_denoise_default_params(&p);
        return !report(fyprt_denoise(m_Ctx, &p, rgba8, nullptr, nullptr), "fyprt_denoise");
    }

    // New (no reference counterpart): the temporal denoiser over the frame Render() just produced (fyprt_denoise_temporal; nullptr = the
    // library's defaults) — in place of Denoise for a moving camera that renders one-sample frames.  The context keeps the history;
    // ResetDenoiseHistory() after a camera cut (scene uploads, geometry updates and resizes drop it themselves).
    bool DenoiseTemporal(const fyprt_temporal_params* params, uint32_t* rgba8) {
        fyprt_temporal_params p;
        if (params) p = *params; else fyprt_denoise_temporal_default_params(&p);
        return !report(fyprt_denoise_temporal(m_Ctx, &p, rgba8, nullptr, nullptr), "fyprt_denoise_temporal");
    }
    void ResetDenoiseHistory() { fyprt_denoise_temporal_reset(m_Ctx); }
    // Object motion (fyprt_denoise_temporal_set_motion): with it on, geometry updates keep the history and the next DenoiseTemporal
    // reprojects every hit through the vertices of the frame denoised before — for dragging a mesh with the temporal denoiser on.
    bool SetDenoiseMotion(bool on) { return !report(fyprt_denoise_temporal_set_motion(m_Ctx, on ? 1 : 0), "fyprt_denoise_temporal_set_motion"); }
    // New (no reference counterpart): denoise the frame Render() just produced at its own size and present it at scale x that size
    // (fyprt_denoise_upscale; nullptr = the library's defaults, scale 2 over the spatial denoiser).  `rgba8` holds scale*width x
    // scale*height pixels.  With params->temporal = 1 the call is the DenoiseTemporal of this frame as well: call one or the other.
    bool DenoiseUpscale(const fyprt_upscale_params* params, uint32_t* rgba8) {
        fyprt_upscale_params p;
        if (params) p = *params; else fyprt_upscale_default_params(&p);
        return !report(fyprt_denoise_upscale(m_Ctx, &p, rgba8, nullptr, nullptr), "fyprt_denoise_upscale");
    }

    // New (no reference counterpart): "Delete Mesh".  Edits the scene (Scene::RemoveMeshesFromScene) and applies the same edit on the device
    // with fyprt_remove_meshes, then stamps the signatures of the reduced scene, so that the next Render() does not upload it.  A removal
    // is not found by comparing signatures: call this instead of editing the arrays.  Before the first upload, or when the library
    // refuses, the scene is edited all the same and the next Render() uploads it.
    template <class SceneT> bool RemoveMeshes(SceneT& scene, const std::vector<uint32_t>& indices) {
        const auto removed = scene.RemoveMeshesFromScene(indices);
        if (!m_HaveScene || isSceneUpdated) { isSceneUpdated = true; m_HaveScene = false; return false; }
        const int rc = fyprt_remove_meshes(m_Ctx, removed.meshes.data(), (uint32_t)removed.meshes.size(), removed.vertexRanges.data());
        if (report(rc, "fyprt_remove_meshes")) { isSceneUpdated = true; m_HaveScene = false; return false; }
        m_StructureSig = StructureSignature(scene, CountsOf(scene)); m_MaterialSig = MaterialSignature(scene);
        KeepMaterialIndices(scene); m_Counts = CountsOf(scene); ++m_Removes;
        return true;
    }
    uint32_t GetSceneRemoveCount() const { return m_Removes; }

    // New (no reference counterpart): meshes that were moved far are taken out of the tree and linked in again where they lie now
    // (fyprt_regraft_meshes) — call it after the Render() that applied their transform edits.  Only the tree moves: the scene, its
    // signatures and the frame state stay as they are.  Returns one report per listed mesh; empty when the library refuses or no scene
    // is on the device yet.  TreeCost() is what tells when it pays: (inner_area + leaf_area) / root_area rises as the tree degrades.
    std::vector<fyprt_append_placement> RegraftMeshes(const std::vector<uint32_t>& indices) {
        std::vector<fyprt_append_placement> reports(indices.size());
        if (!m_HaveScene || report(fyprt_regraft_meshes(m_Ctx, indices.data(), (uint32_t)indices.size(), reports.data()), "fyprt_regraft_meshes")) reports.clear();
        return reports;
    }
    fyprt_tree_cost_sums TreeCost() {
        fyprt_tree_cost_sums cost{};
        if (m_HaveScene) report(fyprt_tree_cost(m_Ctx, &cost), "fyprt_tree_cost");
        return cost;
    }

    void ResetFrameIndex() { fyprt_reset_frame_index(m_Ctx); }
    RenderingSettings& GetSettings() { return m_Settings; }
    uint32_t GetCurrentFrameIndex() const { return fyprt_frame_index(m_Ctx); }
    uint32_t* GetRenderImageDataPtr() const { return const_cast<uint32_t*>(m_RenderImageData.data()); }
    const float* GetAccumulationDataPtr() const { return m_AccumulationData.data(); }
    // The four Resize*Buffers calls of the reference (Renderer.cu:286-419) re-zero the ReSTIR state.
    void ResizeReservoirs(uint32_t w, uint32_t h) { Rezero(w, h); }
    void ResizeDepthBuffers(uint32_t w, uint32_t h) { Rezero(w, h); }
    void ResizeNormalBuffers(uint32_t w, uint32_t h) { Rezero(w, h); }
    void ResizePrimaryHitPayloadBuffers(uint32_t w, uint32_t h) { Rezero(w, h); }
    void FreeDynamicallyAllocatedMemory() { if (m_Ctx) { fyprt_destroy(m_Ctx); m_Ctx = nullptr; } }
    void SetSceneToBeUpdatedFlag(bool flag) { isSceneUpdated = flag; }
    // Called by SceneManager::PerformAllSceneUpdates next to SetSceneToBeUpdatedFlag for a mesh whose transform changed (its
    // Mesh::worldTransformMatrix, column-major) — lets Render() send the matrix instead of the mesh's vertices.  Any other edit
    // that may have moved vertices is reported with NoteOtherSceneEdit() and takes the general path; a material edit (a material's fields, a
    // mesh's material) with NoteMaterialEdit(): it moves no vertex, and Render() finds what changed by comparing with what it uploaded.
    void NoteMeshTransform(uint32_t meshIndex, const float* matrix16) { m_PendingMeshes.push_back(meshIndex); m_PendingTransforms.insert(m_PendingTransforms.end(), matrix16, matrix16 + 16); }
    void NoteOtherSceneEdit() { m_OtherEdits = true; }
    void NoteMaterialEdit() { m_MaterialEdits = true; }
    // Transform edits refit what moved only (tuning key 22 of the context) instead of the whole scene.  Edit detection is unchanged.
    bool SetPartialRefit(bool on) { return m_Ctx && fyprt_set_tuning(m_Ctx, 22, on ? 1 : 0) == FYPRT_OK; }
    // Where an import links its sub-tree (fyprt_set_append_placement): 0 at the root, 1 at the cheapest place by the surface-area rule.
    bool SetAppendPlacement(int mode) { return m_Ctx && fyprt_set_append_placement(m_Ctx, mode) == FYPRT_OK; }
    uint32_t GetTransformUpdateCount() const { return m_TransformUpdates; }
    void SetPresenter(std::function<void(const uint32_t*, uint32_t, uint32_t)> p) { m_Present = std::move(p); }
    const fyprt_frame_stats& GetLastFrameStats() const { return m_LastStats; }
    fyprt_context* GetContext() const { return m_Ctx; }
    uint32_t GetSceneUploadCount() const { return m_Uploads; }
    uint32_t GetSceneRefitCount() const { return m_Refits; }
    uint32_t GetMaterialUpdateCount() const { return m_MaterialUpdates; }
    uint32_t GetSceneAppendCount() const { return m_Appends; }

private:
    // FNV-1a over everything of the scene except vertex positions / normals, in two parts.  Structure: vertex / triangle / mesh / texture
    // counts, triangle vertex indices, mesh ranges, texture identities.  Materials: the table, the material index of every triangle and
    // mesh, the emissive list.
    struct Fnv {
        uint64_t h = 1469598103934665603ull;
        void mix(const void* p, size_t n) { const uint8_t* b = (const uint8_t*)p; for (size_t i = 0; i < n; ++i) { h ^= b[i]; h *= 1099511628211ull; } }
    };
    // (of the scene restricted to `n`: its first n.vertices vertices, n.triangles triangles, ... — the whole scene with CountsOf(scene))
    struct Counts { uint64_t vertices = 0, triangles = 0, meshes = 0, textures = 0; };
    template <class SceneT> static Counts CountsOf(const SceneT& scene) { return Counts{scene.worldVertices.size(), scene.triangles.size(), scene.meshes.size(), scene.textures.size()}; }
    template <class SceneT> static uint64_t StructureSignature(const SceneT& scene, const Counts& n) {
        Fnv f;
        const uint64_t counts[4] = {n.vertices, n.triangles, n.meshes, n.textures};
        f.mix(counts, sizeof counts);
        for (size_t i = 0; i < n.triangles; ++i) { const auto& t = scene.triangles[i]; const uint32_t v[3] = {t.v0, t.v1, t.v2}; f.mix(v, sizeof v); }
        for (size_t i = 0; i < n.meshes; ++i) { const auto& m = scene.meshes[i]; const uint32_t v[2] = {m.indexStart, m.indexCount}; f.mix(v, sizeof v); }
        for (size_t i = 0; i < n.textures; ++i) { const auto& t = scene.textures[i]; const uint64_t v[3] = {(uint64_t)(uintptr_t)t.pixels, t.width, t.height}; f.mix(v, sizeof v); }
        return f.h;
    }
    // Only tails grew on the structure the library holds: the new textures, then the new vertices / triangles / meshes (with their
    // object-space vertices when the upload passed them), and the remembered material indices follow.  false: nothing an append can
    // express, or the library refused — the scene is uploaded again.
    template <class SceneT> bool AppendTails(const SceneT& scene) {
        const Counts now = CountsOf(scene), was = m_Counts;
        if (now.vertices < was.vertices || now.triangles < was.triangles || now.meshes < was.meshes || now.textures < was.textures) return false;
        if (StructureSignature(scene, was) != m_StructureSig) return false;
        if (now.textures > was.textures) {
            std::vector<fyprt_texture> tex;
            for (size_t i = was.textures; i < now.textures; ++i) tex.push_back(fyprt_texture{scene.textures[i].pixels, scene.textures[i].width, scene.textures[i].height});
            if (fyprt_append_textures(m_Ctx, tex.data(), (uint32_t)tex.size()) != FYPRT_OK) return false;
        }
        if (now.meshes > was.meshes || now.triangles > was.triangles || now.vertices > was.vertices) {
            std::vector<fyprt_mesh> meshes; std::vector<uint32_t> first;
            for (size_t i = was.meshes; i < now.meshes; ++i) {
                meshes.push_back(fyprt_mesh{scene.meshes[i].indexStart / 3u, scene.meshes[i].indexCount / 3u, scene.meshes[i].materialIndex});
                first.push_back(scene.meshes[i].vertexStart);
            }
            first.push_back((uint32_t)now.vertices);
            const bool object = m_ObjectVertices && scene.vertices.size() == scene.worldVertices.size();
            const int rc = fyprt_append_meshes(m_Ctx, reinterpret_cast<const fyprt_vertex*>(scene.worldVertices.data()) + was.vertices, (uint32_t)(now.vertices - was.vertices),
                                               scene.triangles.data() + was.triangles, (uint32_t)(now.triangles - was.triangles), (uint32_t)sizeof(scene.triangles[0]),
                                               meshes.data(), (uint32_t)meshes.size(),
                                               object ? reinterpret_cast<const fyprt_vertex*>(scene.vertices.data()) + was.vertices : nullptr, object ? first.data() : nullptr);
            if (rc != FYPRT_OK) return false;
            m_ObjectVertices = object;
            for (size_t i = was.triangles; i < now.triangles; ++i) m_TriMaterial.push_back(scene.triangles[i].materialIndex);
            for (size_t i = was.meshes; i < now.meshes; ++i) m_MeshMaterial.push_back(scene.meshes[i].materialIndex);
        }
        m_Counts = now;
        return true;
    }
    template <class SceneT> static uint64_t MaterialSignature(const SceneT& scene) {
        Fnv f;
        const uint64_t counts[2] = {scene.materials.size(), scene.emissiveTriangles.size()};
        f.mix(counts, sizeof counts);
        for (const auto& t : scene.triangles) { const int32_t v = t.materialIndex; f.mix(&v, 4); }
        for (const auto& m : scene.meshes) { const int32_t v = m.materialIndex; f.mix(&v, 4); }
        if (!scene.materials.empty()) f.mix(scene.materials.data(), scene.materials.size() * sizeof(scene.materials[0]));
        if (!scene.emissiveTriangles.empty()) f.mix(scene.emissiveTriangles.data(), scene.emissiveTriangles.size() * 4);
        return f.h;
    }
    template <class SceneT> void KeepMaterialIndices(const SceneT& scene) {
        m_TriMaterial.resize(scene.triangles.size()); m_MeshMaterial.resize(scene.meshes.size()); m_MaterialCount = scene.materials.size();
        for (size_t i = 0; i < m_TriMaterial.size(); ++i) m_TriMaterial[i] = scene.triangles[i].materialIndex;
        for (size_t i = 0; i < m_MeshMaterial.size(); ++i) m_MeshMaterial[i] = scene.meshes[i].materialIndex;
    }
    // The material part changed, the structure did not: fyprt_update_materials with the whole table, the meshes whose material index
    // differs from what the library holds, and scene.emissiveTriangles exactly as UploadScene passes it.  The call can only say "every
    // triangle of a mesh takes the mesh's material" (SceneManager.cpp:75-79): an edit it cannot express (a lone triangle's material, a
    // shrunken table) returns false, and the scene is uploaded again.
    template <class SceneT> bool UpdateMaterials(const SceneT& scene) {
        if (scene.materials.size() < m_MaterialCount || m_TriMaterial.size() != scene.triangles.size() || m_MeshMaterial.size() != scene.meshes.size()) return false;
        std::vector<uint32_t> meshes; std::vector<int32_t> materials;
        for (size_t m = 0; m < scene.meshes.size(); ++m) {
            const auto& me = scene.meshes[m];
            const bool reassigned = me.materialIndex != m_MeshMaterial[m];
            for (uint32_t t = me.indexStart / 3u; t < me.indexStart / 3u + me.indexCount / 3u; ++t)
                if (scene.triangles[t].materialIndex != (reassigned ? me.materialIndex : m_TriMaterial[t])) return false;
            if (reassigned) { meshes.push_back((uint32_t)m); materials.push_back(me.materialIndex); }
        }
        const int rc = fyprt_update_materials(m_Ctx, reinterpret_cast<const fyprt_material*>(scene.materials.data()), (uint32_t)scene.materials.size(),
                                              meshes.data(), materials.data(), (uint32_t)meshes.size(),
                                              scene.emissiveTriangles.empty() ? nullptr : scene.emissiveTriangles.data(), (uint32_t)scene.emissiveTriangles.size());
        if (rc != FYPRT_OK) return false;
        KeepMaterialIndices(scene);
        return true;
    }
    template <class SceneT> bool UploadScene(SceneT& scene) {                                 // SceneToGPU, Scene_GPU.cpp:6-81
        fyprt_scene_desc d{};
        d.vertices = reinterpret_cast<const fyprt_vertex*>(scene.worldVertices.data()); d.vertex_count = (uint32_t)scene.worldVertices.size();
        d.triangles = scene.triangles.data(); d.triangle_count = (uint32_t)scene.triangles.size();
        d.triangle_stride = (uint32_t)sizeof(scene.triangles[0]);
        d.materials = reinterpret_cast<const fyprt_material*>(scene.materials.data()); d.material_count = (uint32_t)scene.materials.size();
        std::vector<fyprt_mesh> meshes(scene.meshes.size());
        for (size_t i = 0; i < meshes.size(); ++i)
            meshes[i] = fyprt_mesh{scene.meshes[i].indexStart / 3u, scene.meshes[i].indexCount / 3u, scene.meshes[i].materialIndex};
        d.meshes = meshes.data(); d.mesh_count = (uint32_t)meshes.size();
        std::vector<fyprt_texture> tex(scene.textures.size());
        for (size_t i = 0; i < tex.size(); ++i) tex[i] = fyprt_texture{scene.textures[i].pixels, scene.textures[i].width, scene.textures[i].height};
        d.textures = tex.data(); d.texture_count = (uint32_t)tex.size();
        d.emissive_triangles = scene.emissiveTriangles.empty() ? nullptr : scene.emissiveTriangles.data();
        d.emissive_count = (uint32_t)scene.emissiveTriangles.size();
        d.light_trees = nullptr;                      // the library builds them (LightTree.cpp restated)
        if (report(fyprt_upload_scene(m_Ctx, &d), "fyprt_upload_scene")) return false;
        // object-space vertices + mesh vertex ranges: what fyprt_update_transforms needs (Scene::vertices, Mesh::vertexStart / vertexCount)
        m_ObjectVertices = false;
        if (scene.vertices.size() == scene.worldVertices.size()) {
            std::vector<uint32_t> first(scene.meshes.size() + 1, (uint32_t)scene.vertices.size());
            for (size_t i = 0; i < scene.meshes.size(); ++i) first[i] = scene.meshes[i].vertexStart;
            m_ObjectVertices = fyprt_set_object_vertices(m_Ctx, reinterpret_cast<const fyprt_vertex*>(scene.vertices.data()), (uint32_t)scene.vertices.size(), first.data()) == FYPRT_OK;
        }
        return true;
    }
    void Rezero(uint32_t w, uint32_t h) { m_Width = m_Height = 0; OnResize(w, h); }
    bool report(int rc, const char* what) {          // the reference prints and keeps going (Renderer.cu:29-47)
        if (rc == FYPRT_OK) return false;
        std::fprintf(stderr, "%s error: %s\n", what, fyprt_last_error(m_Ctx));
        return true;
    }
    RenderingSettings m_Settings;
    fyprt_context* m_Ctx = nullptr;
    uint32_t m_Width = 0, m_Height = 0;
    std::vector<uint32_t> m_RenderImageData;
    std::vector<float> m_AccumulationData;
    bool isSceneUpdated = true;
    bool m_HaveScene = false; uint64_t m_StructureSig = 0, m_MaterialSig = 0; uint32_t m_Uploads = 0, m_Refits = 0, m_TransformUpdates = 0, m_MaterialUpdates = 0, m_Appends = 0, m_Removes = 0;
    Counts m_Counts; bool m_ObjectVertices = false;                                         // what was uploaded: the counts an append starts from; with object-space vertices
    std::vector<uint32_t> m_PendingMeshes; std::vector<float> m_PendingTransforms; bool m_OtherEdits = false, m_MaterialEdits = false;
    std::vector<int32_t> m_TriMaterial, m_MeshMaterial; size_t m_MaterialCount = 0;     // what the library holds (UpdateMaterials)
    std::function<void(const uint32_t*, uint32_t, uint32_t)> m_Present;
    fyprt_frame_stats m_LastStats{};
};

}  // namespace fyprt_host
