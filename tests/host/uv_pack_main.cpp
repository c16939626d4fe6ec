// uv_pack_main.cpp -- the streamed weight images of ngf_uv_pack.hpp on the CPU (no HIP, no GPU): the plan of the packed inverse network with
// every segment, forward and transposed, filled by uv_pack_value -- what ngf_uv_inverse_create does on the host and uvit_pack_kernel on the
// device -- and the fp32 images of ngf_uv.hip's UvPacker at four of its shapes through the same slot map.  tests/test_uv_pack_cpu.py compiles
// it with the host compiler (and the address / undefined-behaviour sanitizers), runs it and compares what it wrote with a numpy restatement.
//
//   uv_pack_main WEIGHTS OUTDIR
//
// WEIGHTS: raw float32 -- for D = 2, then D = 3, the ten tensors of the inverse network in descriptor order (weight [out][in], bias [out] of
// linear1 D -> 64, linear2 64 -> 512, two hidden 512 -> 512, last_linear 512 -> 3); then UvPacker's: w [256][63], w [128][64], w [3][256],
// w [256][295], b [256], b [3].
// OUTDIR: receives inv_d2.pack, inv_d3.pack (the whole packed set: forward set, transposed set, zero block) and uvp_NAME.pack, raw bytes.
// stdout: `seg dD INDEX KIND DST COUNT OUT_F IN_F SO SI NT HID` per segment and `at dD NAME VALUE` per offset / count of the plan.
#include <cstdio>
#include <string>
#include <vector>

#include "ngf_uv_pack.hpp"

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

// an fp32 image as UvPacker::image fills it: the slot map says whose each word is, imap where its input comes from
template <typename F>
static std::vector<float> uvp_image(int kind, int NT, size_t count, const std::vector<float> &W, int out_f, int in_f, F imap)
{
    std::vector<float> img(count);
    for (size_t idx = 0; idx < count; ++idx) {
        const UvPackSlot s = uv_pack_slot(kind, NT, (int)idx);
        if (kind >= kUvPackBias) { img[idx] = s.o < out_f ? W[s.o] : 0.0f; continue; }
        const int i = imap(s.t, s.kq);
        img[idx] = (s.o < out_f && i >= 0 && i < in_f) ? W[(size_t)s.o * in_f + i] : 0.0f;
    }
    return img;
}

int main(int argc, char **argv)
{
    if (argc != 3) { fprintf(stderr, "usage: %s WEIGHTS OUTDIR\n", argv[0]); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 1; }
    const std::string outdir = argv[2];
    for (int D = 2; D <= 3; ++D) {
        const UvInvShape shape = uv_inverse_shape(D);
        std::vector<float> W[NGF_UV_INVERSE_LAYERS], B[NGF_UV_INVERSE_LAYERS];
        const float *w[NGF_UV_INVERSE_LAYERS], *b[NGF_UV_INVERSE_LAYERS];
        for (int l = 0; l < NGF_UV_INVERSE_LAYERS; ++l) {
            if (!take(f, W[l], (size_t)shape.out_f[l] * shape.in_f[l]) || !take(f, B[l], shape.out_f[l])) { fprintf(stderr, "%s is too short\n", argv[1]); return 1; }
            w[l] = W[l].data(); b[l] = B[l].data();
        }
        const UvInvPlan P = uv_inverse_plan(D, w, b);
        std::vector<float> buf(P.floats, 0.0f);          // (the trainer clears its buffer once: the zero block is no segment)
        for (int s = 0; s < P.nseg; ++s) {
            const UvPackSeg &S = P.seg[s];
            if (S.dst < 0 || S.count < 0 || S.dst + S.count > P.floats) { fprintf(stderr, "d%d: segment %d leaves the buffer\n", D, s); return 1; }
            for (int idx = 0; idx < S.count; ++idx) buf[S.dst + idx] = uv_pack_value(S, idx);
            printf("seg d%d %d %d %d %d %d %d %d %d %d %d\n", D, s, S.kind, S.dst, S.count, S.out_f, S.in_f, S.so, S.si, S.NT, S.hid);
        }
        const struct { const char *name; int v; } at[] = {
            {"w1", P.fwd.w1}, {"b1", P.fwd.b1}, {"w2", P.fwd.w2}, {"b2", P.fwd.b2}, {"wh", P.fwd.wh}, {"bh", P.fwd.bh}, {"wo", P.fwd.wo}, {"bo", P.fwd.bo},
            {"to", P.dx.to}, {"th", P.dx.th}, {"t2", P.dx.t2}, {"t1", P.dx.t1}, {"zb", P.dx.zb},
            {"nfwd", P.nfwd}, {"nseg", P.nseg}, {"fwd_floats", P.fwd_floats}, {"floats", P.floats}};
        for (const auto &a : at) printf("at d%d %s %d\n", D, a.name, a.v);
        if (!dump(outdir + "/inv_d" + std::to_string(D) + ".pack", buf)) { fprintf(stderr, "cannot write to %s\n", argv[2]); return 1; }
    }
    std::vector<float> w63, w64, w3, w295, b256, b3;
    bool ok = take(f, w63, 256 * 63) && take(f, w64, 128 * 64) && take(f, w3, 3 * 256) && take(f, w295, 256 * 295) && take(f, b256, 256) && take(f, b3, 3);
    ok = ok && fgetc(f) == EOF;
    fclose(f);
    if (!ok) { fprintf(stderr, "%s does not hold exactly the floats of the two networks and the six UvPacker tensors\n", argv[1]); return 1; }
    auto nat = [](int t, int kq) { return uv_pack_input(t, kq, false); };
    auto hid = [](int t, int kq) { return uv_pack_input(t, kq, true); };
    auto mixed = [](int t, int kq) { return t < 64 ? uv_pack_input(t, kq, true) : 256 + 4 * (t - 64) + kq; };      // ngf_uv_create's 295-input layer
    ok = dump(outdir + "/uvp_dense_256x63.pack", uvp_image(kUvPackDense, 16, 16 * 16 * 64, w63, 256, 63, nat)) &&
         dump(outdir + "/uvp_dense_128x64.pack", uvp_image(kUvPackDense, 8, 16 * 8 * 64, w64, 128, 64, hid)) &&
         dump(outdir + "/uvp_out_3x256.pack", uvp_image(kUvPackOut, 0, 64 * 64, w3, 3, 256, hid)) &&
         dump(outdir + "/uvp_dense_256x295.pack", uvp_image(kUvPackDense, 16, 76 * 16 * 64, w295, 256, 295, mixed)) &&
         dump(outdir + "/uvp_bias_256.pack", uvp_image(kUvPackBias, 16, 16 * 16, b256, 256, 0, nat)) &&
         dump(outdir + "/uvp_bias4_3.pack", uvp_image(kUvPackBias4, 0, 4, b3, 3, 0, nat));
    if (!ok) { fprintf(stderr, "cannot write to %s\n", argv[2]); return 1; }
    return 0;
}
