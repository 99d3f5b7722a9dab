// Nothing throws or aborts across the rt_scene_* C-ABI: this program replaces the
// global operator new so that the N-th allocation after arming throws std::bad_alloc, and calls each
// entry point that can allocate with N = 0, 1, 2, ... until the call first succeeds.  Every failing
// call must return RT_ERR_OUT_OF_MEMORY or RT_ERR_IO and leave a scene that rt_scene_free takes;
// an exception that left an entry point would end the process in std::terminate.  Host code only:
//   g++ -std=c++17 -I include tools/scene_alloc_check.cpp <the library's host sources> -lz
// It writes its own inputs (the smallest that reach each entry's code) into a temporary directory.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <functional>
#include <new>
#include <string>
#include <unistd.h>

#include "../include/rt_scene.h"

static long g_countdown = -1;   // < 0: not armed; 0: the next allocation fails
static bool fail_now() { return g_countdown >= 0 && g_countdown-- == 0; }
void* operator new(size_t n) {
    if (fail_now()) throw std::bad_alloc();
    if (void* p = std::malloc(n ? n : 1)) return p;
    throw std::bad_alloc();
}
void* operator new[](size_t n) { return operator new(n); }
void* operator new(size_t n, const std::nothrow_t&) noexcept { return fail_now() ? nullptr : std::malloc(n ? n : 1); }
void* operator new[](size_t n, const std::nothrow_t& t) noexcept { return operator new(n, t); }
void operator delete(void* p) noexcept { std::free(p); }
void operator delete[](void* p) noexcept { std::free(p); }
void operator delete(void* p, size_t) noexcept { std::free(p); }
void operator delete[](void* p, size_t) noexcept { std::free(p); }

static std::string g_dir;
static void write_file(const std::string& name, const std::string& text) {
    FILE* f = std::fopen((g_dir + "/" + name).c_str(), "wb");
    if (!f || std::fwrite(text.data(), 1, text.size(), f) != text.size()) std::exit(2);
    std::fclose(f);
}

static const char* kObj = "mtllib tiny.mtl\no quad\nv 0 0 0\nv 1 0 0\nv 1 1 0\nv 0 1 0\nvt 0 0\nvt 1 0\nvt 1 1\nvt 0 1\n"
                          "usemtl m\nf 1/1 2/2 3/3 4/4\n";
static const char* kMtl = "newmtl m\nKd 0.5 0.25 0.125\nmap_Kd tex.png\n";
static const char* kUsda = R"(#usda 1.0
def SkelRoot "R"
{
    def Skeleton "Skel"
    {
        uniform token[] joints = ["a", "a/b"]
        uniform matrix4d[] bindTransforms = [((1, 0, 0, 0), (0, 1, 0, 0), (0, 0, 1, 0), (0, 0, 0, 1)), ((1, 0, 0, 0), (0, 1, 0, 0), (0, 0, 1, 0), (0, 1, 0, 1))]
        uniform matrix4d[] restTransforms = [((1, 0, 0, 0), (0, 1, 0, 0), (0, 0, 1, 0), (0, 0, 0, 1)), ((1, 0, 0, 0), (0, 1, 0, 0), (0, 0, 1, 0), (0, 1, 0, 1))]
    }
    def Mesh "Tri"
    {
        int[] faceVertexCounts = [3]
        int[] faceVertexIndices = [0, 1, 2]
        point3f[] points = [(0, 0, 0), (1, 0, 0), (0, 1, 0)]
        int[] primvars:skel:jointIndices = [0, 1, 1] (
            interpolation = "vertex"
        )
        float[] primvars:skel:jointWeights = [1, 1, 1] (
            interpolation = "vertex"
        )
        rel skel:skeleton = </R/Skel>
        rel material:binding = </R/Mat>
    }
    def Material "Mat"
    {
        token outputs:surface.connect = </R/Mat/S.outputs:surface>
        def Shader "S"
        {
            uniform token info:id = "UsdPreviewSurface"
            color3f inputs:diffuseColor = (0.5, 0.25, 0.125)
            token outputs:surface
        }
    }
}
)";

static const float kZero[3] = {0, 0, 0};
static int g_bad = 0;

// setup(scene) runs unarmed on a fresh scene, then call(scene) with the N-th allocation failing
static void check(const char* entry, const std::function<bool(rt_scene*)>& setup,
                  const std::function<rt_status(rt_scene*)>& call) {
    long oom = 0, io = 0;
    for (long n = 0;; ++n) {
        rt_scene* s = nullptr;
        if (rt_scene_new(&s) != RT_OK || !setup(s)) {
            std::printf("%-26s SETUP FAILED: %s\n", entry, s ? rt_scene_last_error(s) : "");
            ++g_bad;
            rt_scene_free(s);
            return;
        }
        g_countdown = n;
        const rt_status st = call(s);
        g_countdown = -1;
        if (st == RT_ERR_OUT_OF_MEMORY) ++oom;
        else if (st == RT_ERR_IO) ++io;
        else if (st != RT_OK) {
            std::printf("%-26s N=%ld: status %d (%s)\n", entry, n, (int)st, rt_scene_last_error(s));
            ++g_bad;
        }
        rt_scene_free(s);
        if (st == RT_OK) {
            std::printf("%-26s first success at N=%ld; %ld x RT_ERR_OUT_OF_MEMORY, %ld x RT_ERR_IO\n", entry, n, oom, io);
            return;
        }
        if (g_bad) return;
    }
}

int main() {
    char tmpl[] = "/tmp/scene_alloc_check.XXXXXX";
    if (!mkdtemp(tmpl)) return 2;
    g_dir = tmpl;
    const uint8_t texels[16] = {255, 0, 0, 255, 0, 255, 0, 255, 0, 0, 255, 255, 255, 255, 255, 255};
    if (rt_write_png((g_dir + "/tex.png").c_str(), texels, 2, 2) != RT_OK) return 2;
    write_file("tiny.mtl", kMtl);
    for (const char* n : {"tiny.obj", "plane.obj", "sphere.obj", "plane-back.obj"}) write_file(n, kObj);   // preset c1's models
    write_file("tri.usda", kUsda);
    const std::string obj = g_dir + "/tiny.obj", usda = g_dir + "/tri.usda", png = g_dir + "/tex.png";

    auto nothing = [](rt_scene*) { return true; };
    auto with_obj = [&](rt_scene* s) { return rt_scene_add_obj(s, obj.c_str(), kZero, kZero, 1.0f, nullptr) == RT_OK; };
    auto with_usd = [&](rt_scene* s) { return rt_scene_add_usd(s, usda.c_str(), kZero, kZero, 1.0f, nullptr) == RT_OK; };

    check("rt_scene_add_obj", nothing, [&](rt_scene* s) { return rt_scene_add_obj(s, obj.c_str(), kZero, kZero, 1.0f, nullptr); });
    check("rt_scene_add_usd", nothing, [&](rt_scene* s) { return rt_scene_add_usd(s, usda.c_str(), kZero, kZero, 1.0f, nullptr); });
    check("rt_scene_add_procedural", nothing,
          [&](rt_scene* s) { return rt_scene_add_procedural(s, "bunny", nullptr, kZero, kZero, 1.0f, nullptr); });
    check("rt_scene_preset", nothing, [&](rt_scene*) {
        rt_scene* p = nullptr;
        const rt_status st = rt_scene_preset("c1", g_dir.c_str(), &p, nullptr);
        g_countdown = -1;
        if (st != RT_OK && p && !*rt_scene_last_error(p)) {   // a failed preset hands the scene and its error back
            std::printf("rt_scene_preset: status %d without an error text\n", (int)st);
            ++g_bad;
        }
        rt_scene_free(p);
        return st;
    });
    check("rt_scene_get_desc", with_obj, [&](rt_scene* s) { rt_scene_desc d; return rt_scene_get_desc(s, &d); });
    check("rt_scene_add_texture", nothing, [&](rt_scene* s) { uint32_t id; return rt_scene_add_texture(s, texels, 2, 2, &id); });
    check("rt_scene_load_texture", nothing, [&](rt_scene* s) { uint32_t id; return rt_scene_load_texture(s, png.c_str(), &id); });
    check("rt_scene_bind_texture", with_obj, [&](rt_scene* s) { return rt_scene_bind_texture(s, 0, 0, 1, 0); });
    check("rt_scene_joint_matrices", with_usd, [&](rt_scene* s) {
        float out[2 * 16];
        uint32_t jc = 0;
        return rt_scene_joint_matrices(s, 0, 0.37, out, 2, &jc);
    });
    check("rt_scene_set_lights", nothing, [&](rt_scene* s) {
        Light l[3] = {};
        return rt_scene_set_lights(s, l, 3);
    });

    for (const char* n : {"tiny.obj", "plane.obj", "sphere.obj", "plane-back.obj", "tiny.mtl", "tri.usda", "tex.png"})
        std::remove((g_dir + "/" + n).c_str());
    rmdir(g_dir.c_str());
    std::printf(g_bad ? "FAILED\n" : "ok: every failing call returned an error status and left a freeable scene\n");
    return g_bad ? 1 : 0;
}
