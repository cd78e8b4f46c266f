// An import through the facade: what MainLayer does for "Import Mesh" and "Import Texture" (WalnutApp.cpp:668-693 ->
// Scene::CreateNewMeshInScene, Scene.cpp:241-290; WalnutApp.cpp:739-754 -> Scene::CreateNewTextureInScene, Scene.cpp:228-239), on the
// harness's Cornell scene.  Renderer A renders, a texture and a small tessellated sheet are pushed onto the end of the scene's arrays,
// the emissive list is refreshed (InitSceneEmissiveTriangles) and A renders again — the facade sends the tails with
// fyprt_append_textures / fyprt_append_meshes instead of uploading the scene again.  Renderer B is constructed fresh on the grown scene
// and renders the same frame.  The two acceleration structures differ (A's took a sub-tree at its root), so the frames agree except
// where two triangles are hit at exactly the same distance: the share of identical pixels is printed and must pass the bar of the
// refit test for a differently built tree.  History-free settings (no accumulation).  Exit status 1 below the bar.
// A third argument sets A's placement mode (Renderer::SetAppendPlacement, default 0); the kind of place the import took is printed.
#include <cmath>
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
    Material sheet; sheet.albedo = {0.9f, 0.8f, 0.2f};
    scene.materials = {white, red, green, light, sheet};
    quad(scene, {-1, -1, 1}, {1, -1, 1}, {1, -1, -1}, {-1, -1, -1}, {0, 1, 0}, 0);
    quad(scene, {-1, 1, -1}, {1, 1, -1}, {1, 1, 1}, {-1, 1, 1}, {0, -1, 0}, 0);
    quad(scene, {-1, -1, -1}, {1, -1, -1}, {1, 1, -1}, {-1, 1, -1}, {0, 0, 1}, 0);
    quad(scene, {-1, -1, 1}, {-1, -1, -1}, {-1, 1, -1}, {-1, 1, 1}, {1, 0, 0}, 1);
    quad(scene, {1, -1, -1}, {1, -1, 1}, {1, 1, 1}, {1, 1, -1}, {-1, 0, 0}, 2);
    quad(scene, {-0.25f, 0.999f, -0.25f}, {0.25f, 0.999f, -0.25f}, {0.25f, 0.999f, 0.25f}, {-0.25f, 0.999f, 0.25f}, {0, -1, 0}, 3);
    scene.InitSceneEmissiveTriangles();
}
// the imported mesh: an n x n sheet of quads with a gentle wave, in object space around the origin
static void importSheet(Scene& scene, int n, int mat) {
    std::vector<Vertex> v; std::vector<uint32_t> idx;
    for (int j = 0; j <= n; ++j)
        for (int i = 0; i <= n; ++i) {
            const float x = (float)i / (float)n - 0.5f, y = (float)j / (float)n - 0.5f;
            v.push_back({{x, y, 0.05f * std::sin(7.0f * x + 3.0f * y)}, {0, 0, 1}, {x + 0.5f, y + 0.5f}});
        }
    for (int j = 0; j < n; ++j)
        for (int i = 0; i < n; ++i) {
            const uint32_t a = (uint32_t)(j * (n + 1) + i), b = a + 1, c = a + (uint32_t)n + 1, d = c + 1;
            for (uint32_t k : {a, b, d, a, d, c}) idx.push_back(k);
        }
    scene.AddNewMeshToScene(v, idx, vec3{0.1f, -0.2f, 0.6f}, vec3{-20.0f, 25.0f, 0.0f}, vec3{0.8f, 0.8f, 0.8f}, mat);
}
static void settings(Renderer& r, int tech, uint32_t seed) {
    RenderingSettings& s = r.GetSettings();
    s.currentSamplingTechnique = (SamplingTechniqueEnum)tech; s.lightBounces = 4; s.skyColor[0] = s.skyColor[1] = s.skyColor[2] = 0.0f;
    s.toAccumulate = false; s.useTemporalReuse = false; s.useSpatialReuse = true; s.randSeed = seed;
}

int main(int argc, char** argv) {
    const uint32_t W = argc > 1 ? std::atoi(argv[1]) : 128, H = argc > 2 ? std::atoi(argv[2]) : 80;
    const int placement = argc > 3 ? std::atoi(argv[3]) : 0;
    const double bar = 0.97;                                              // identical pixels for a differently built tree
    std::vector<uint32_t> pixels(8 * 8);
    for (size_t i = 0; i < pixels.size(); ++i) pixels[i] = 0xFF000000u | (uint32_t)(i * 0x030507u);
    bool allPass = true;
    for (int tech : {(int)COSINE_WEIGHTED_SAMPLING, (int)NEE}) {
        const char* name = tech == NEE ? "NEE" : "cosine";
        Scene scene; cornell(scene);
        Camera camera(45.0f, 0.1f, 100.0f);
        camera.OnResize(W, H); camera.SetPosition({0, 0, 3.4f});
        Renderer a(0);
        a.OnResize(W, H);
        if (!a.SetAppendPlacement(placement)) { std::printf("placement mode %d refused\n", placement); return 1; }
        scene.sceneManager.PerformAllSceneUpdates(scene, a);          // drains the 20 default queue entries
        settings(a, tech, 2); a.Render(scene, camera);
        // the import, as the UI does it: a texture, a mesh, the emissive list again, the scene-updated flag
        Texture t; t.pixels = pixels.data(); t.width = 8; t.height = 8; t.fileName = "generated";
        scene.textures.push_back(t);
        importSheet(scene, 12, 4);
        scene.InitSceneEmissiveTriangles();
        a.SetSceneToBeUpdatedFlag(true);
        settings(a, tech, 3); a.Render(scene, camera);
        Renderer b(0);
        b.OnResize(W, H);
        settings(b, tech, 3); b.Render(scene, camera);
        const size_t n = (size_t)W * H;
        size_t same = 0;
        for (size_t p = 0; p < n; ++p) same += std::memcmp(a.GetAccumulationDataPtr() + p * 4, b.GetAccumulationDataPtr() + p * 4, 16) == 0;
        const double share = (double)same / (double)n;
        const bool pass = b.GetSceneUploadCount() == 1 && a.GetSceneUploadCount() == 1 && a.GetSceneAppendCount() == 1 && share > bar;
        std::printf("%s scene uploads (A): %u\n%s scene appends (A): %u\n%s material updates (A): %u\n%s triangles: %zu\n%s identical pixels: %.4f\n",
                    name, a.GetSceneUploadCount(), name, a.GetSceneAppendCount(), name, a.GetMaterialUpdateCount(), name, scene.triangles.size(), name, share);
        fyprt_append_placement pl{};
        const bool reported = fyprt_last_append_placement(a.GetContext(), &pl) == FYPRT_OK && pl.mode == (uint32_t)placement;
        std::printf("%s placement mode: %u\n%s placement kind: %u\n%s levels after: %u\n", name, pl.mode, name, pl.kind, name, pl.levels_after);
        allPass = allPass && pass && reported;
    }
    return allPass ? 0 : 1;
}
