// Host-side check of cf_align_faces_frame's argument validation and frame staging layout under AddressSanitizer + UBSan: a stand-alone
// program (no GPU is touched, no kernel is launched) that drives every refusal of cf::align_frame_check and walks the staging layout of
// every format over odd and extreme sizes.  Build and run from the repository root:
//   C=lightweight-face-detection-centernet_amd/csrc
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Iinclude -I$C -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//         -Xarch_host -fno-sanitize-recover=undefined tools/align_frame_hostcheck.hip $C/cf_align_frame.hip $C/cf_align.hip $C/cf_redact.hip \
//         -o build/align_frame_hostcheck && build/align_frame_hostcheck          (after mkdir -p build)
// Prints "ok: N refusals, M layouts" and exits 0; any sanitizer report or wrong answer is a non-zero exit.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "centerface_hip.h"
#include "cf_kernels.h"

using namespace cf;

static int g_refusals = 0, g_fail = 0;

struct Args {
    int size = 112, chip = 0, rgb = 0, mpi = 0, format = CF_FRAME_BGR, on_device = 0, B = 2, h = 32, w = 32, pitch0 = 96, pitch1 = 32;
    const void* const* planes = nullptr;
    const float* tmpl = nullptr;
};

static const char* run(const Args& a) {
    AlignFrameParams p{};
    return align_frame_check(p, a.size, a.chip, a.rgb, 0.0f, 1.0f, a.tmpl, a.mpi, a.format, a.planes, a.on_device, a.B, a.h, a.w, a.pitch0, a.pitch1);
}

static void refuse(const Args& a, const char* word, int line) {
    const char* why = run(a);
    if (!why || !strstr(why, word)) { fprintf(stderr, "line %d: wanted a refusal naming '%s', got '%s'\n", line, word, why ? why : "(accepted)"); ++g_fail; }
    ++g_refusals;
}
#define REFUSE(a, word) refuse(a, word, __LINE__)

int main() {
    // plane tables on the heap, exactly 3 * B entries: a read past them is the sanitizer's to find
    std::vector<unsigned char> bytes(64);
    const int B = 2;
    std::vector<const void*> full(3 * B, bytes.data()), two(3 * B, bytes.data()), one(3 * B, nullptr), odd(3 * B, bytes.data() + 2);
    for (int b = 0; b < B; ++b) { two[3 * b + 2] = nullptr; one[3 * b] = bytes.data(); }
    Args ok; ok.planes = full.data();
    if (const char* why = run(ok)) { fprintf(stderr, "the base case was refused: %s\n", why); return 1; }
    { Args a = ok; a.planes = one.data(); if (run(a)) { fprintf(stderr, "BGR needs one plane only\n"); return 1; } }
    { Args a = ok; a.format = CF_YUV_NV12; a.pitch0 = 32; a.planes = two.data(); if (run(a)) { fprintf(stderr, "NV12 needs two planes only\n"); return 1; } }
    { Args a = ok; a.h = 31; a.w = 33; a.pitch0 = 99; if (run(a)) { fprintf(stderr, "odd BGR sides are fine\n"); return 1; } }
    { Args a = ok; a.h = 8192; a.w = 8192; a.pitch0 = 3 * 8192; if (run(a)) { fprintf(stderr, "8192 is the largest side\n"); return 1; } }
    for (int size : {0, 12, 15, 18, 113, 516, 1024, -112}) { Args a = ok; a.size = size; REFUSE(a, "size"); }
    for (int chip : {-1, 2, 7}) { Args a = ok; a.chip = chip; REFUSE(a, "chip format"); }
    { Args a = ok; a.mpi = -1; REFUSE(a, "max_per_image"); }
    for (int f : {-1, 5, 99, -2147483647 - 1, 2147483647}) { Args a = ok; a.format = f; REFUSE(a, "format"); }
    for (int f : {CF_YUV_NV12, CF_YUV_NV21, CF_YUV_I420, CF_YUV_YV12}) {
        Args a = ok; a.format = f; a.pitch0 = 40; a.pitch1 = 40;
        { Args b = a; b.h = 31; REFUSE(b, "even"); }
        { Args b = a; b.w = 31; REFUSE(b, "even"); }
        { Args b = a; b.pitch0 = 31; REFUSE(b, "pitch0"); }
        { Args b = a; b.pitch1 = (f == CF_YUV_NV12 || f == CF_YUV_NV21) ? 31 : 15; REFUSE(b, "pitch1"); }
        { Args b = a; b.pitch1 = -4; REFUSE(b, "pitch1"); }
        { Args b = a; b.planes = one.data(); REFUSE(b, "null plane"); }
        if (f >= CF_YUV_I420) { Args b = a; b.planes = two.data(); REFUSE(b, "null plane"); }
        { Args b = a; b.on_device = 1; b.pitch1 = 42; REFUSE(b, "multiples of 4"); }
    }
    for (int side : {0, 1, -1, -32, 8193, 8194, 2147483647, -2147483647 - 1}) {
        { Args a = ok; a.h = side; REFUSE(a, "[2, 8192]"); }
        { Args a = ok; a.w = side; a.pitch0 = 2147483647; REFUSE(a, "[2, 8192]"); }
    }
    for (int p : {95, 0, -96, -2147483647 - 1}) { Args a = ok; a.pitch0 = p; REFUSE(a, "pitch0"); }
    for (int nb : {0, -1, -2147483647 - 1}) { Args a = ok; a.B = nb; REFUSE(a, "B must"); }
    { Args a = ok; a.planes = nullptr; REFUSE(a, "null frame table"); }
    { Args a = ok; std::vector<const void*> t(full); t[3] = nullptr; a.planes = t.data(); REFUSE(a, "null plane"); }
    { Args a = ok; a.on_device = 1; a.planes = odd.data(); REFUSE(a, "4-byte aligned"); }
    { Args a = ok; a.on_device = 1; a.pitch0 = 98; REFUSE(a, "multiples of 4"); }
    // the staging layout of the host form: planes in order, 4-byte aligned, rows of at least the row bytes, nothing overlapping, and
    // the last byte of the last plane inside `one`
    int layouts = 0;
    for (int f = CF_YUV_NV12; f <= CF_FRAME_BGR; ++f)
        for (int h : {2, 3, 150, 151, 1080, 8191, 8192})
            for (int w : {2, 3, 202, 203, 1920, 8191, 8192}) {
                if (f != CF_FRAME_BGR && ((h | w) & 1)) continue;
                const RedactStage st = redact_stage_layout(f, h, w);
                const bool bgr = f == CF_FRAME_BGR, il = f == CF_YUV_NV12 || f == CF_YUV_NV21;
                const size_t end0 = (size_t)st.pitch0 * h, end1 = st.off1 + (size_t)st.pitch1 * st.rows1, end2 = st.off2 + (size_t)st.pitch1 * st.rows1;
                bool good = st.row0 == (bgr ? 3 * w : w) && st.pitch0 >= st.row0 && !(st.pitch0 & 3) && !(st.pitch1 & 3) && st.off1 == end0 && !(st.one & 3);
                if (bgr) good = good && st.one == end0;
                else if (il) good = good && st.row1 == w && st.pitch1 >= w && st.rows1 == h / 2 && st.one == end1;
                else good = good && st.row1 == w / 2 && st.pitch1 >= w / 2 && st.rows1 == h / 2 && st.off2 == end1 && st.one == end2;
                // the kernel's last BGR dword (h * pitch0 / 4 - 1) ends exactly at the plane's end
                if (bgr) good = good && ((size_t)h * st.pitch0 / 4 - 1) * 4 + 4 == end0;
                if (!good) { fprintf(stderr, "staging layout of format %d, %d x %d is wrong\n", f, w, h); ++g_fail; }
                ++layouts;
            }
    if (g_fail) return 1;
    printf("ok: %d refusals, %d layouts\n", g_refusals, layouts);
    return 0;
}
