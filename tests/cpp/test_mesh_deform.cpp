// The deforming-mesh calls through the C++ host mirror (softwarerenderer_amd/cpp/Rasterizer.hpp): known answers that are exact in
// every numerics model (halves of small integers), the pose seen by a draw, and the mirror's error behaviour.
//   make -C tests/cpp -f mesh_deform.mk && tests/cpp/test_mesh_deform
#include <cstdio>
#include <cstring>
#include <vector>

#include "Rasterizer.hpp"

using namespace SoftwareRenderer;

static Shaders::VertexInput vertex(float x, float y, float z, float nx, float ny, float nz) {
    Shaders::VertexInput v{};
    v.position[0] = x; v.position[1] = y; v.position[2] = z;
    v.uv[0] = 0.25f; v.uv[1] = 0.75f;
    v.normal[0] = nx; v.normal[1] = ny; v.normal[2] = nz;
    v.color[0] = 1.0f; v.color[1] = 0.5f; v.color[2] = 0.25f; v.color[3] = 1.0f;
    return v;
}

static int expect(bool ok, const char* what) {
    if (!ok) printf("FAILED: %s\n", what);
    return ok ? 0 : 1;
}

int main() {
    int fails = 0;
    try {
        Device dev(0);
        const std::vector<uint16_t> idx = { 0, 1, 2 };
        const std::vector<Shaders::VertexInput> va = { vertex(-1, -1, 0.5f, 0, 0, 1), vertex(1, -1, 0.5f, 0, 0, 1), vertex(0, 1, 0.5f, 0, 0, 1) };
        std::vector<Shaders::VertexInput> vb = va;
        for (auto& v : vb) { v.position[0] += 4.0f; v.color[0] = 0.0f; v.normal[1] = 2.0f; }
        Mesh a(dev, va, idx), b(dev, vb, idx);
        Mesh dst = a.Like();
        fails += expect(std::memcmp(dst.Read().data(), va.data(), va.size() * sizeof va[0]) == 0, "Like copies the vertices");

        dst.BlendFrom(a, b, 0.5f);
        std::vector<Shaders::VertexInput> got = dst.Read();
        for (size_t i = 0; i < got.size(); ++i) {
            fails += expect(got[i].position[0] == va[i].position[0] + 2.0f && got[i].position[1] == va[i].position[1], "blend: position");
            fails += expect(got[i].normal[1] == 1.0f && got[i].normal[2] == 1.0f, "blend: the normal is not renormalised");
            fails += expect(got[i].color[0] == 0.5f && got[i].uv[1] == 0.75f, "blend: colour and uv");
        }

        // two joints: identity, and a translation by (2, 0, 0); weights (1/2, 1/2, 0, 0): x moves by one, the normal stays (0, 0, 1)
        Matrix4x4 ident{}; ident[0] = ident[5] = ident[10] = ident[15] = 1.0f;
        Matrix4x4 shift = ident; shift[12] = 2.0f;
        a.SetSkin({ 0, 1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0 }, { 0.5f, 0.5f, 0, 0, 0.5f, 0.5f, 0, 0, 0.5f, 0.5f, 0, 0 });
        dst.SkinFrom(a, { ident, shift });
        got = dst.Read();
        for (size_t i = 0; i < got.size(); ++i) {
            fails += expect(got[i].position[0] == va[i].position[0] + 1.0f && got[i].position[1] == va[i].position[1] && got[i].position[2] == 0.5f, "skin: position");
            fails += expect(got[i].normal[0] == 0.0f && got[i].normal[1] == 0.0f && got[i].normal[2] == 1.0f, "skin: normal");
            fails += expect(got[i].color[1] == 0.5f && got[i].uv[0] == 0.25f, "skin: colour and uv are copied");
        }

        // a draw sees the pose: the triangle moved to x in [0, 2], so the frame's left half stays clear
        MainWindow w(dev, 64, 64);
        w.ClearDepthBuffer(); w.ClearColorBuffer({ 0, 0, 0, 1 });
        ShaderProgram flat{};
        flat.program = Shaders::Program::FlatColor;
        Rasterizer::RenderMesh(w, dst, ident, ident, ident, flat, Rasterizer::CullMode::None);
        fails += expect(w.GetPixel(16, 32)[0] == 0.0f, "the bind pose's place is empty");
        fails += expect(w.GetPixel(48, 40)[0] == 1.0f, "the posed triangle is drawn");

        // refusals throw std::invalid_argument, as the mirror's other argument errors do
        bool threw = false;
        try { a.BlendFrom(a, b, 0.5f); } catch (const std::invalid_argument&) { threw = true; }
        fails += expect(threw, "a destination that is a key frame is refused");
        threw = false;
        try { dst.SkinFrom(b, { ident, shift }); } catch (const std::invalid_argument&) { threw = true; }
        fails += expect(threw, "a source without skin attributes is refused");
        dst.BlendFrom(a, b, 0.0f);
        fails += expect(std::memcmp(dst.Read().data(), va.data(), va.size() * sizeof va[0]) == 0, "a valid call after the refusals");
    } catch (const std::exception& e) {
        printf("exception: %s\n", e.what());
        return 2;
    }
    printf(fails ? "FAILED\n" : "ALL OK\n");
    return fails ? 1 : 0;
}
