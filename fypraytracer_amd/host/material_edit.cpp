// A material edit through the facade: what MainLayer does when the UI changes a material or assigns another one to a mesh
// (WalnutApp.cpp:690-723 -> SceneManager::PerformAllSceneUpdates, SceneManager.cpp:10-17, :69-85), on the harness's Cornell scene.
// Renderer A renders, the light's emission power is changed and the red wall is assigned the light material through the SceneManager
// queues, the emissive list is refreshed (InitSceneEmissiveTriangles), and A renders again — the facade applies the edit with
// fyprt_update_materials instead of uploading the scene again.  Renderer B is constructed fresh on the edited scene and renders the
// same frame.  History-free settings (NEE without accumulation; ReSTIR DI without temporal reuse), so the two frames must be identical.
// Prints per technique the upload and material-update counts of A and whether the images are identical; exit status 1 if not.
#include <cstdlib>
#include "HostTypes.h"
#include "Renderer.h"
using namespace fyprt_host;

static void quad(Scene& s, vec3 a, vec3 b, vec3 c, vec3 d, vec3 n, int mat) {
    std::vector<Vertex> v = {{a, n, {0, 0}}, {b, n, {1, 0}}, {c, n, {1, 1}}, {d, n, {0, 1}}};
    s.AddNewMeshToScene(v, {0, 1, 2, 0, 2, 3}, mat);
}
static void cornell(Scene& scene) {
    Material white; white.albedo = {1, 1, 1}; Material red; red.albedo = {1, 0, 0}; Material green; green.albedo = {0, 1, 0};
    Material light; light.albedo = {1, 1, 1}; light.emissionColor = {1, 1, 1}; light.emissionPower = 40.0f;   // WalnutApp.cpp:56-59
    scene.materials = {white, red, green, light};
    quad(scene, {-1, -1, 1}, {1, -1, 1}, {1, -1, -1}, {-1, -1, -1}, {0, 1, 0}, 0);
    quad(scene, {-1, 1, -1}, {1, 1, -1}, {1, 1, 1}, {-1, 1, 1}, {0, -1, 0}, 0);
    quad(scene, {-1, -1, -1}, {1, -1, -1}, {1, 1, -1}, {-1, 1, -1}, {0, 0, 1}, 0);
    quad(scene, {-1, -1, 1}, {-1, -1, -1}, {-1, 1, -1}, {-1, 1, 1}, {1, 0, 0}, 1);       // mesh 3: the red wall
    quad(scene, {1, -1, -1}, {1, -1, 1}, {1, 1, 1}, {1, 1, -1}, {-1, 0, 0}, 2);
    quad(scene, {-0.25f, 0.999f, -0.25f}, {0.25f, 0.999f, -0.25f}, {0.25f, 0.999f, 0.25f}, {-0.25f, 0.999f, 0.25f}, {0, -1, 0}, 3);
    scene.InitSceneEmissiveTriangles();
}
static void settings(Renderer& r, int tech, uint32_t seed) {
    RenderingSettings& s = r.GetSettings();
    s.currentSamplingTechnique = (SamplingTechniqueEnum)tech; s.lightBounces = 4; s.skyColor[0] = s.skyColor[1] = s.skyColor[2] = 0.0f;
    s.toAccumulate = false; s.useTemporalReuse = false; s.useSpatialReuse = true; s.randSeed = seed;
}

int main(int argc, char** argv) {
    const uint32_t W = argc > 1 ? std::atoi(argv[1]) : 128, H = argc > 2 ? std::atoi(argv[2]) : 96;
    bool allSame = true;
    for (int tech : {(int)NEE, (int)RESTIR_DI}) {
        const char* name = tech == NEE ? "NEE" : "ReSTIR DI";
        Scene scene; cornell(scene);
        Camera camera(45.0f, 0.1f, 100.0f);
        camera.OnResize(W, H); camera.SetPosition({0, 0, 3.4f});
        Renderer a(0);
        a.OnResize(W, H);
        scene.sceneManager.PerformAllSceneUpdates(scene, a);          // drains the 20 default queue entries
        settings(a, tech, 2); a.Render(scene, camera);
        // the edit, as the UI queues it (WalnutApp.cpp:702-715)
        scene.materials[3].emissionPower = 15.0f; scene.sceneManager.materialsToUpdate.push_back(3u);
        scene.meshes[3].materialIndex = 3; scene.sceneManager.meshesToUpdate.emplace_back(false, true, 3u);
        scene.sceneManager.PerformAllSceneUpdates(scene, a);
        scene.InitSceneEmissiveTriangles();
        settings(a, tech, 3); a.Render(scene, camera);
        Renderer b(0);
        b.OnResize(W, H);
        settings(b, tech, 3); b.Render(scene, camera);
        const size_t n = (size_t)W * H;
        const bool same = b.GetSceneUploadCount() == 1 && std::memcmp(a.GetRenderImageDataPtr(), b.GetRenderImageDataPtr(), n * 4) == 0 &&
                          std::memcmp(a.GetAccumulationDataPtr(), b.GetAccumulationDataPtr(), n * 16) == 0;
        std::printf("%s scene uploads (A): %u\n%s material updates (A): %u\n%s device refits (A): %u\n%s emissive triangles: %zu\n%s images identical: %s\n",
                    name, a.GetSceneUploadCount(), name, a.GetMaterialUpdateCount(), name, a.GetSceneRefitCount(), name, scene.emissiveTriangles.size(), name, same ? "yes" : "no");
        allSame = allSame && same;
    }
    return allSame ? 0 : 1;
}
