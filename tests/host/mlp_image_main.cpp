// mlp_image_main.cpp -- builds every MLP image of ngf_mlp_image.hpp on the CPU (no HIP, no GPU).  tests/test_mlp_image_cpu.py compiles it with
// the host compiler (and the address / undefined-behaviour sanitizers), runs it and compares what it wrote with tests/golden/mlp_images.npz;
// tests/golden/make_golden_mlp_images.py writes that golden with it.
//
//   mlp_image_main WEIGHTS OUTDIR [--time N]
//
// WEIGHTS: raw float32, the tensors of the two models at the only sizes ngf_field_create accepts, in this order --
//   TriPlane (F = 144): basis [F][F], w1p [64][F], w1 [64][F + 15], b1 [64], w2 [64][64], b2 [64], w3 [3][64], b3 [3], dw1 [48], db1 [1]
//   InfoInv  (F = 216):               w1p [64][F], w1 [64][F + 15], b1 [64], w2 [64][64], b2 [64], w3 [3][64], b3 [3],
//                                     dw1 [32][72], db1 [32], dw2 [32][32], db2 [32], dw3 [32], db3 [1]
// OUTDIR: receives NAME.img and (where the formulation streams a matrix) NAME.pack as raw bytes, one pair per configuration.
// stdout: one line `section NAME SECTION OFFSET COUNT` (floats) per part of every image, from the layout structs -- the test names a
// mismatch and finds the pad slots with them; with --time N one line `time NAME MICROSECONDS`, the best of N builds.
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "ngf_mlp_image.hpp"

using namespace ngf;

static bool take(FILE *f, std::vector<float> &v, size_t n)
{
    v.resize(n);
    return fread(v.data(), sizeof(float), n, f) == n;
}

static bool dump(const std::string &path, const std::vector<float> &v)
{
    FILE *f = fopen(path.c_str(), "wb");
    if (!f) return false;
    const bool ok = fwrite(v.data(), sizeof(float), v.size(), f) == v.size();
    return fclose(f) == 0 && ok;
}

struct Section { const char *name; int offset; };

// the parts of a colour image, in offset order, closed by its TOTAL
template <typename L>
static std::vector<Section> colour_sections(int w1)
{
    return {{"W1", w1}, {"W2", L::W2}, {"B1", L::B1}, {"B2", L::B2}, {"W3", L::W3}, {"B3", L::B3}, {nullptr, L::TOTAL}};
}
template <typename D>
static std::vector<Section> density_sections()
{
    return {{"dens.D1", D::D1}, {"dens.D2", D::D2}, {"dens.B1", D::B1}, {"dens.B2", D::B2}, {"dens.W3", D::W3}, {"dens.B3", D::B3}, {nullptr, D::TOTAL}};
}

struct Config {
    const char *name;
    int model, flags;
    std::vector<Section> colour, density;
};

int main(int argc, char **argv)
{
    if (argc != 3 && !(argc == 5 && !strcmp(argv[3], "--time"))) {
        fprintf(stderr, "usage: %s WEIGHTS OUTDIR [--time N]\n", argv[0]);
        return 2;
    }
    const int reps = argc == 5 ? atoi(argv[4]) : 0;
    FieldWeights tri, ii;
    FILE *f = fopen(argv[1], "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 1; }
    bool ok = take(f, tri.basis, 144 * 144) && take(f, tri.w1p, 64 * 144) && take(f, tri.w1, 64 * 159) && take(f, tri.b1, 64) && take(f, tri.w2, 64 * 64) &&
              take(f, tri.b2, 64) && take(f, tri.w3, 3 * 64) && take(f, tri.b3, 3) && take(f, tri.dw1, 48) && take(f, tri.db1, 1);
    ok = ok && take(f, ii.w1p, 64 * 216) && take(f, ii.w1, 64 * 231) && take(f, ii.b1, 64) && take(f, ii.w2, 64 * 64) && take(f, ii.b2, 64) &&
         take(f, ii.w3, 3 * 64) && take(f, ii.b3, 3) && take(f, ii.dw1, 32 * 72) && take(f, ii.db1, 32) && take(f, ii.dw2, 32 * 32) && take(f, ii.db2, 32) &&
         take(f, ii.dw3, 32) && take(f, ii.db3, 1);
    ok = ok && fgetc(f) == EOF;
    fclose(f);
    if (!ok) { fprintf(stderr, "%s does not hold exactly the floats of the two models\n", argv[1]); return 1; }

    const Config configs[7] = {
        {"tri_fp32", NGF_MODEL_TRIPLANE, 0, colour_sections<MlpLayout16<48>>(MlpLayout16<48>::W1), {}},
        {"tri_bake", NGF_MODEL_TRIPLANE, NGF_F_BAKE_DENSITY | NGF_F_BAKE_COLOR, colour_sections<MlpLayout16Baked>(MlpLayout16Baked::W1V), {}},
        {"tri_bake_bf16", NGF_MODEL_TRIPLANE, NGF_F_BAKE_DENSITY | NGF_F_BAKE_COLOR | NGF_F_SPLIT_BF16, colour_sections<MlpLayout16BakedBf16>(MlpLayout16BakedBf16::W1V), {}},
        {"tri_bf16", NGF_MODEL_TRIPLANE, NGF_F_SPLIT_BF16, colour_sections<MlpLayoutBf16>(MlpLayoutBf16::W1), {}},
        {"tri_nofold", NGF_MODEL_TRIPLANE, NGF_F_NO_FOLD, colour_sections<MlpLayout16NoFold>(MlpLayout16NoFold::W1), {}},
        {"ii_fp32", NGF_MODEL_INFOINV, 0, colour_sections<MlpLayout16<72>>(MlpLayout16<72>::W1), density_sections<InfoInvDensLayout>()},
        {"ii_bf16", NGF_MODEL_INFOINV, NGF_F_SPLIT_BF16, colour_sections<MlpLayoutBf16II>(MlpLayoutBf16II::W1), density_sections<InfoInvDensLayoutBf16>()},
    };
    for (const Config &c : configs) {
        const FieldWeights &W = c.model == NGF_MODEL_TRIPLANE ? tri : ii;
        std::vector<float> img, pack;
        build_field_images(c.model, c.flags, W, img, pack);
        const int colour_total = c.colour.back().offset, total = colour_total + (c.density.empty() ? 0 : c.density.back().offset);
        if ((size_t)total != img.size()) { fprintf(stderr, "%s: %zu floats built, the layouts say %d\n", c.name, img.size(), total); return 1; }
        for (size_t s = 0; s + 1 < c.colour.size(); ++s)
            printf("section %s %s %d %d\n", c.name, c.colour[s].name, c.colour[s].offset, c.colour[s + 1].offset - c.colour[s].offset);
        for (size_t s = 0; s + 1 < c.density.size(); ++s)
            printf("section %s %s %d %d\n", c.name, c.density[s].name, colour_total + c.density[s].offset, c.density[s + 1].offset - c.density[s].offset);
        const std::string base = std::string(argv[2]) + "/" + c.name;
        if (!dump(base + ".img", img) || (!pack.empty() && !dump(base + ".pack", pack))) { fprintf(stderr, "cannot write %s.*\n", base.c_str()); return 1; }
        if (reps > 0) {
            double best = 1e30;
            for (int r = 0; r < reps; ++r) {
                const auto t0 = std::chrono::steady_clock::now();
                build_field_images(c.model, c.flags, W, img, pack);
                const double us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
                if (us < best) best = us;
            }
            printf("time %s %.1f\n", c.name, best);
        }
    }
    return 0;
}
