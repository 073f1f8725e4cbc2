// Per-op C-ABI entry points (cf_op_*): each runs ONE production kernel, or one product sequence of them, on the caller's host arrays, so
// the parity tests can check it in isolation against the oracle, the reference's golden vectors or a float64 restatement.  The layer ops take
// host NCHW float32 tensors as the torch op they replace would (the layout conversion happens on the device around the kernel); the decode,
// row and tile ops take the row tables of the ABI; the frame ops take pitched host frames, staged as the blocking product calls stage them;
// the sequence ops (track, follow, scene, lookback, best shot) step one launch's pointers through the frames of a fresh state object.  There
// is no CPU compute path here.  Every entry point reads the same way -- validation (before any device is touched), declarations (`Scope`'s
// verbs below), launches, `result`.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "centerface_hip.h"
#include "cf_common.h"
#include "cf_kernels.h"

using namespace cf;

namespace {

thread_local std::string g_op_error;

// the refusal of entry point `who`
int fail(const char* who, const char* why) { g_op_error = std::string(who) + ": " + why; return CF_EINVAL; }

// Host frames staged by Scope::stage: n frames back to back in cf_frame.h's staging layout, and their device plane table
struct Staged {
    RedactStage st{};
    int format = 0, n = 0, h = 0, w = 0, pitch0 = 0, pitch1 = 0;      // the host frames' own pitches
    const void* const* host = nullptr;
    uint8_t* base = nullptr;
    std::vector<const void*> table;
    // the geometry of a launch over B of the staged frames (the staged pitches), and the table from frame `first` on
    FrameGeo geo(int B) const { return FrameGeo{format, B, h, w, st.pitch0, st.pitch1}; }
    const void* const* planes(size_t first = 0) const { return table.data() + 3 * first; }
};

// The device side of one entry point: a stream, the allocations, the first error, and the result copies.  Nothing runs after an error
// (`run`), and the caller's arrays are written only once every launch has completed (`result`).
struct Scope {
    hipStream_t s = nullptr;
    std::vector<void*> ptrs;
    struct Back { void* host; const void* dev; size_t bytes; };
    std::vector<Back> backs;      // the result copies, in the order of their declaration
    hipError_t err = hipSuccess;
    explicit Scope(int device) {
        err = hipSetDevice(device);
        if (err == hipSuccess) err = hipStreamCreateWithFlags(&s, hipStreamNonBlocking);   // never the legacy stream (see upload() in cf_runtime.hip)
    }
    ~Scope() {
        if (s) { hipStreamSynchronize(s); hipStreamDestroy(s); }
        for (void* p : ptrs) hipFree(p);
    }
    bool ok() const { return err == hipSuccess; }
    // every launch and every HIP call of an entry point: f() runs only while nothing has failed, and its error is kept
    template <typename F> void run(F&& f) { if (err == hipSuccess) err = f(); }
    void* alloc(size_t bytes) {
        if (err != hipSuccess) return nullptr;
        void* p = nullptr;
        err = hipMalloc(&p, bytes + 256);
        // zeroed body; the tail pad (kernels with clamped loads may read a few bytes past a buffer) holds 0xFF bytes, a NaN in every
        // storage type, so that a read past the end shows in the result instead of meeting whatever the allocator held
        if (err == hipSuccess) { ptrs.push_back(p); if (bytes) hipMemsetAsync(p, 0, bytes, s); hipMemsetAsync((char*)p + bytes, 0xFF, 256, s); }
        return p;
    }
    void* alloc_nan(size_t bytes) {
        void* p = alloc(bytes);
        run([&] { return hipMemsetAsync(p, 0xFF, bytes, s); });      // an element the kernel skips comes back as NaN
        return p;
    }
    void* up(const void* host, size_t bytes) {
        void* p = alloc(bytes);
        run([&] { return hipMemcpyAsync(p, host, bytes, hipMemcpyHostToDevice, s); });
        return p;
    }
    // result() copies `bytes` at dev to host
    void back(void* host, const void* dev, size_t bytes) { if (bytes) backs.push_back(Back{host, dev, bytes}); }
    // n elements: scratch (zeroed), an input, an output (zeroed), an output that starts as the caller's buffer -- so that rows the kernel
    // leaves alone come back with the caller's values.  A null output is scratch: nothing comes back.
    template <typename T> T* make(size_t n) { return (T*)alloc(n * sizeof(T)); }
    template <typename T> T* in(const T* host, size_t n) { return (T*)up(host, n * sizeof(T)); }
    template <typename T> T* upv(const std::vector<T>& v) { return in(v.data(), v.size()); }
    template <typename T> T* out(T* host, size_t n) {
        T* p = make<T>(n);
        if (host) back(host, p, n * sizeof(T));
        return p;
    }
    template <typename T> T* inout(T* host, size_t n) {
        T* p = host ? in(host, n) : make<T>(n);
        if (host) back(host, p, n * sizeof(T));
        return p;
    }
    // host f32 NCHW -> device T NHWC
    void* to_nhwc(int dtype, const float* host, int B, int C, int H, int W) {
        size_t n = (size_t)B * C * H * W;
        float* src = in(host, n);
        void* dst = alloc(n * elem_size(dtype));
        run([&] { return launch_nchw_to_nhwc(s, dtype, src, dst, B, C, H, W); });
        return dst;
    }
    // host f32 NCHW -> device T in pixel-block order [m / 32][C / P][m % 32][P], padded to whole 32-pixel blocks as the engine's buffers are
    void* to_blocked(int dtype, const float* host, int B, int C, int H, int W) {
        size_t n = (size_t)B * C * H * W;
        float* src = in(host, n);
        void* dst = alloc(blocked_bytes(dtype, B, C, H, W));
        run([&] { return launch_nchw_to_blocked(s, dtype, src, dst, B, C, H, W); });
        return dst;
    }
    static size_t blocked_bytes(int dtype, int B, int C, int H, int W) {
        return (((size_t)B * H * W + 31) / 32 * 32) * C * elem_size(dtype);
    }
    // device T pixel-block order -> host f32 NCHW (an output like any other: result() copies the converted temporary)
    void blocked_to_host_nchw(int dtype, const void* dev, float* host, int B, int C, int H, int W) {
        float* tmp = out(host, (size_t)B * C * H * W);
        run([&] { return launch_blocked_to_nchw(s, dtype, dev, tmp, B, C, H, W); });
    }
    // device T NHWC -> host f32 NCHW (likewise)
    void to_host_nchw(int dtype, const void* dev, float* host, int B, int C, int H, int W) {
        float* tmp = out(host, (size_t)B * C * H * W);
        run([&] { return launch_nhwc_to_nchw(s, dtype, dev, tmp, B, C, H, W); });
    }
    // n host frames -> the staging layout on the device, as cf_op_redact stages them (the row bytes only; pitches rounded up to 4)
    Staged stage(int format, const void* const* host_planes, int n, int h, int w, int pitch0, int pitch1) {
        Staged fr;
        fr.st = redact_stage_layout(format, h, w);
        fr.format = format; fr.n = n; fr.h = h; fr.w = w; fr.pitch0 = pitch0; fr.pitch1 = pitch1; fr.host = host_planes;
        fr.base = (uint8_t*)alloc(fr.st.one * n);
        fr.table = stage_table(fr.st, fr.base, format, n);
        run([&] { return redact_stage_copy(s, fr.st, format, host_planes, n, h, pitch0, pitch1, fr.base, true); });
        return fr;
    }
    // ... and back into the host frames, behind the launches that changed them
    void unstage(const Staged& fr) {
        run([&] { return redact_stage_copy(s, fr.st, fr.format, fr.host, fr.n, fr.h, fr.pitch0, fr.pitch1, fr.base, false); });
    }
    // The end of every entry point: the declared outputs come back once the whole sequence ran (nothing is written otherwise), and the list
    // is cleared (cf_op_decode_threshold_ex comes here twice on one Scope).
    int result(const char* what) {
        run([&] { return hipStreamSynchronize(s); });
        for (const Back& b : backs) run([&] { return hipMemcpyAsync(b.host, b.dev, b.bytes, hipMemcpyDeviceToHost, s); });
        run([&] { return hipStreamSynchronize(s); });
        backs.clear();
        if (err == hipSuccess) return CF_OK;
        g_op_error = std::string(what) + ": " + hipGetErrorString(err);
        return CF_EHIP;
    }
};

// Packed rows: image b owns the next counts[b] rows.  count_rows: nullptr with the largest count (at least 1) in *rows (may be null) and
// the sum in *N, or `refusal` where a count is negative or above `limit`.
const char* count_rows(const int32_t* counts, int B, int limit, const char* refusal, int* rows, long long* N) {
    int most = 1;
    *N = 0;
    for (int b = 0; b < B; ++b) {
        if (counts[b] < 0 || counts[b] > limit) return refusal;
        most = std::max(most, (int)counts[b]); *N += counts[b];
    }
    if (rows) *rows = most;
    return nullptr;
}
// ... spread to [B][rows][width] (zero where an image has fewer) -- the layout the decode leaves behind, so that the launches address the
// rows exactly as the engine's do; no rows (src null): an empty vector
template <typename T> std::vector<T> spread(const T* src, const int32_t* counts, int B, int rows, int width) {
    std::vector<T> v(src ? (size_t)B * rows * width : 0, T(0));
    for (long long b = 0, at = 0; src && b < B; at += counts[b], ++b)
        if (counts[b]) memcpy(&v[(size_t)b * rows * width], src + at * width, (size_t)counts[b] * width * sizeof(T));
    return v;
}

bool bad_dtype(int d) { return d != CF_F32 && d != CF_BF16 && d != CF_F32_SPLIT; }

void fold(const float* bn /*[4][C]: weight,bias,mean,var*/, int C, float eps, std::vector<double>& sc, std::vector<double>& sh) {
    sc.resize(C); sh.resize(C);
    for (int c = 0; c < C; ++c) {
        sc[c] = (double)bn[c] / std::sqrt((double)bn[3 * C + c] + (double)eps);
        sh[c] = (double)bn[C + c] - (double)bn[2 * C + c] * sc[c];
    }
}

// explicit maps (NCHW) -> the 16-float head record layout the decode kernels read
std::vector<float> make_records(const float* hm, const float* wh, const float* reg, const float* lm, int B, int h, int w) {
    const size_t HW = (size_t)h * w;
    std::vector<float> rec((size_t)B * HW * 16, 0.0f);
    for (int b = 0; b < B; ++b)
        for (size_t i = 0; i < HW; ++i) {
            float* r = &rec[((size_t)b * HW + i) * 16];
            r[0] = hm[(size_t)b * HW + i];
            if (wh) { r[1] = wh[((size_t)b * 2 + 0) * HW + i]; r[2] = wh[((size_t)b * 2 + 1) * HW + i]; }
            if (lm) for (int c = 0; c < 10; ++c) r[3 + c] = lm[((size_t)b * 10 + c) * HW + i];
            if (reg) { r[13] = reg[((size_t)b * 2 + 0) * HW + i]; r[14] = reg[((size_t)b * 2 + 1) * HW + i]; }
        }
    return rec;
}

// launch_mbconv(p).  An A/B build (-DCF_X5_TIMING, tools/ab_build.sh) launches `reps` times first and times one more launch with events;
// with `counters` it points the kernel (*slot) at tn zeroed 64-bit counters, where every wave leaves four phase cycle sums, and hands the
// time, the number of waves that wrote any and the four totals to print(ms, waves, sum), which writes them to stderr.
template <typename Slot, typename Print>
void launch_mbconv_timed(Scope& sc, int dtype, MbParams& p, Slot* slot, bool counters, size_t tn, int reps, Print print) {
    auto launch = [&] { return launch_mbconv(sc.s, dtype, p); };
#ifdef CF_X5_TIMING
    unsigned long long* tdev = sc.make<unsigned long long>(tn);
    if (counters) { (void)hipMemsetAsync(tdev, 0, tn * 8, sc.s); *slot = tdev; }
    for (int rep = 0; rep < reps; ++rep) sc.run(launch);
    hipEvent_t e0, e1; (void)hipEventCreate(&e0); (void)hipEventCreate(&e1);
    (void)hipEventRecord(e0, sc.s);
    sc.run(launch);
    (void)hipEventRecord(e1, sc.s); (void)hipStreamSynchronize(sc.s);
    float ms = 0; (void)hipEventElapsedTime(&ms, e0, e1);
    if (!counters) return;
    std::vector<unsigned long long> th(tn);
    (void)hipMemcpy(th.data(), tdev, tn * 8, hipMemcpyDeviceToHost);
    double sum[4] = {0, 0, 0, 0}; size_t nw = 0;
    for (size_t i = 0; i + 3 < tn; i += 4) if (th[i] | th[i + 1] | th[i + 2] | th[i + 3]) { for (int k = 0; k < 4; ++k) sum[k] += (double)th[i + k]; ++nw; }
    print(ms, nw, sum);
#else
    sc.run(launch);
#endif
}

// Host frames of cf_op_align_frame, cf_op_cut_tiles and cf_op_fit -> their device plane table.  Every plane is copied up whole (rows x pitch
// bytes), each into its own allocation, so the caller's padding bytes sit beside the pixels on the device and Scope's 0xFF pad follows every plane.
std::vector<const void*> up_planes(Scope& sc, int format, const void* const* hp, int B, int h, int pitch0, int pitch1) {
    std::vector<const void*> dev((size_t)3 * B, nullptr);
    for (int b = 0; b < B; ++b)
        for (int k = 0; k < frame_planes(format); ++k) dev[3 * b + k] = sc.up(hp[3 * b + k], k == 0 ? (size_t)h * pitch0 : (size_t)(h / 2) * pitch1);
    return dev;
}

// What the two align ops share: the N packed landmark rows and their counts as an align launch reads them, and its outputs, of which the
// chips and matrices of the rows taken (all of them, or at most max_per_image of an image) come back
void align_rows(Scope& sc, AlignParams& a, const float* lms, const int32_t* counts, int B, long long N, const cf_align_opts* o, void* chips, double* matrices) {
    const size_t one = align_chip_bytes(o->size, o->format);
    a.lms = sc.in(lms, (size_t)N * 10); a.lms_stride = 0; a.rows_cap = INT_MAX;
    a.counts = sc.in(counts, B);
    a.chips = sc.alloc(one * N);
    a.mats = matrices ? sc.make<double>((size_t)N * 6) : nullptr;
    a.offsets = nullptr; a.cap_faces = (int)N;
    size_t n = (size_t)N;
    if (o->max_per_image > 0) { n = 0; for (int b = 0; b < B; ++b) n += std::min(counts[b], o->max_per_image); }
    sc.back(chips, a.chips, one * n);
    if (matrices) sc.back(matrices, a.mats, n * 6 * sizeof(double));
}

// What cf_op_redact and cf_op_blur share, on host frames (in place): the rest of the validation (`why`: what the entry point's own check
// found), the packed box rows spread on the host, the staging of the frames, and launch(sc, staged geometry, staged planes, faces) between
// the copy up and the copy down.
template <typename Launch>
int op_on_faces(const char* who, const char* why, int device, const FrameGeo& g, const cf_planes_rw* frames, const float* boxes,
                const int32_t* counts, int H, int W, Launch launch) {
    static_assert(sizeof(cf_planes_rw) == 3 * sizeof(void*), "cf_planes_rw is a table of three addresses");
    const void* const* host_planes = reinterpret_cast<const void* const*>(frames);
    if (!why) why = redact_check_planes(g.format, host_planes, g.B, 0, g.pitch0, g.pitch1);
    if (!why && (!counts || H < 1 || W < 1)) why = "null counts, or H / W below 1";
    int rows = 1;
    long long N = 0;
    if (!why) why = count_rows(counts, g.B, 1 << 20, "a count is negative or above 2^20", &rows, &N);
    if (!why && N > 0 && !boxes) why = "null boxes";
    if (why) return fail(who, why);
    if (N == 0) return CF_OK;
    const std::vector<float> sb = spread(boxes, counts, g.B, rows, 4);
    Scope sc(device);
    const FaceList f{sc.upv(sb), rows, sc.in(counts, g.B), rows, rows, H, W};
    const Staged fr = sc.stage(g.format, host_planes, g.B, g.h, g.w, g.pitch0, g.pitch1);
    launch(sc, fr.geo(g.B), fr.planes(), f);
    sc.unstage(fr);
    return sc.result(who);
}

}  // namespace

namespace cf {
// what cf_op_last_error reports, for an entry point of cf_runtime.hip that was called without a context
void op_error_set(const char* text) { g_op_error = text; }
}  // namespace cf

extern "C" {

const char* cf_op_last_error(void) { return g_op_error.c_str(); }
const char* cf_op_last_kernel(void) { return last_kernel_tag(); }

// Page-locked host memory without a context (hipHostMalloc, portable: every device may DMA from it): what cfa.pinned_empty hands out.
int cf_pinned_alloc(uint64_t bytes, void** hptr) {
    if (!hptr || bytes == 0) { g_op_error = "cf_pinned_alloc: null pointer or zero size"; return CF_EINVAL; }
    *hptr = nullptr;
    const hipError_t e = hipHostMalloc(hptr, bytes, hipHostMallocPortable);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        *hptr = nullptr;
        g_op_error = std::string("hipHostMalloc: ") + hipGetErrorString(e);
        return e == hipErrorOutOfMemory ? CF_ENOMEM : CF_EHIP;
    }
    return CF_OK;
}
int cf_pinned_free(void* hptr) {
    if (!hptr) return CF_OK;
    const hipError_t e = hipHostFree(hptr);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        g_op_error = std::string("hipHostFree: ") + hipGetErrorString(e);
        return CF_EHIP;
    }
    return CF_OK;
}

// Page-lock memory the caller already owns (a mapped frame pool, a shared-memory segment) so that cf_forward / cf_forward_resized /
// cf_forward_images read it by asynchronous DMA, without the staging copy into cf_host_alloc memory.  Costs a page-table walk per call
// (~0.1 ms per MB): for buffers that are reused, not for one-shot images.  Whole pages of a mapping of its own only (the header's
// contract): round 5 registered numpy heap arrays, and the GPU faulted on them once the C library had trimmed and regrown its heap
// underneath (the SIGABRT of GPUTEST_r05).
int cf_host_register(void* hptr, uint64_t bytes) {
    if (!hptr || bytes == 0) { g_op_error = "cf_host_register: null pointer or zero size"; return CF_EINVAL; }
    if ((reinterpret_cast<uintptr_t>(hptr) & 4095u) || (bytes & 4095u)) {
        g_op_error = "cf_host_register: the range must be whole pages (pointer and size multiples of 4096) of a mapping of its own -- not malloc / numpy heap memory; use cf_pinned_alloc";
        return CF_EINVAL;
    }
    const hipError_t e = hipHostRegister(hptr, bytes, hipHostRegisterPortable | hipHostRegisterMapped);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        g_op_error = std::string("hipHostRegister: ") + hipGetErrorString(e);
        return e == hipErrorOutOfMemory ? CF_ENOMEM : CF_EHIP;
    }
    return CF_OK;
}
int cf_host_unregister(void* hptr) {
    if (!hptr) { g_op_error = "cf_host_unregister: null pointer"; return CF_EINVAL; }
    const hipError_t e = hipHostUnregister(hptr);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        g_op_error = std::string("hipHostUnregister: ") + hipGetErrorString(e);
        return CF_EHIP;
    }
    return CF_OK;
}

// What cf_op_dwconv and cf_op_dw_pick refuse before anything else, and the output size.  The padded input must hold one window: C's division
// truncates, so (H + pad - k) / stride + 1 alone would call a 2-row input under a 3 x 3 stride-2 window one output row.
static bool dw_args(int dtype, int C, int H, int W, int k, int stride, int pad_lo, int pad_hi, int act, int* Ho, int* Wo) {
    if (bad_dtype(dtype) || (C % 8) || (k != 3 && k != 5) || (stride != 1 && stride != 2) || (act != 0 && act != 1)) return false;
    if (H < 1 || W < 1 || (long long)H + pad_lo + pad_hi < k || (long long)W + pad_lo + pad_hi < k) return false;
    *Ho = (H + pad_lo + pad_hi - k) / stride + 1; *Wo = (W + pad_lo + pad_hi - k) / stride + 1;
    return true;
}
static DwParams dw_shape(int B, int C, int H, int W, int Ho, int Wo, int k, int stride, int pad_lo, int act) {
    DwParams p{};
    p.B = B; p.C = C; p.H = H; p.W = W; p.Ho = Ho; p.Wo = Wo; p.k = k; p.s = stride; p.pad_lo = pad_lo; p.act = act;
    return p;
}
int cf_op_dwconv(int device, int dtype, const float* x, const float* w, const float* bias, float* y,
                 int B, int C, int H, int W, int k, int stride, int pad_lo, int pad_hi, int act) {
    int Ho = 0, Wo = 0;
    if (!x || !w || !y || !dw_args(dtype, C, H, W, k, stride, pad_lo, pad_hi, act, &Ho, &Wo)) return CF_EINVAL;
    Scope sc(device);
    std::vector<float> wp((size_t)k * k * C);
    dw_pack_weights(w, C, k, wp.data());
    DwParams p = dw_shape(B, C, H, W, Ho, Wo, k, stride, pad_lo, act);
    p.x = sc.to_nhwc(dtype, x, B, C, H, W);
    p.w = sc.upv(wp);
    p.bias = bias ? sc.in(bias, C) : nullptr;
    p.y = sc.alloc_nan((size_t)B * Ho * Wo * C * elem_size(dtype));
    sc.run([&] { return launch_dw(sc.s, dtype, p); });
    sc.to_host_nchw(dtype, p.y, y, B, C, Ho, Wo);
    return sc.result("cf_op_dwconv");
}
// launch_dw's choice for the shape cf_op_dwconv would hand it (dw_choose: the host half of launch_dw, no device)
int cf_op_dw_pick(int dtype, int B, int C, int H, int W, int k, int stride, int pad_lo, int pad_hi, int act, int has_bias,
                  int out[16], char* tag, int tag_len) {
    if (bad_dtype(dtype) || !out || B < 1 || (tag && tag_len < 1)) return CF_EINVAL;
    for (int i = 0; i < 16; ++i) out[i] = 0;
    if (tag) tag[0] = 0;
    int Ho = 0, Wo = 0;
    if (!dw_args(dtype, C, H, W, k, stride, pad_lo, pad_hi, act, &Ho, &Wo)) return CF_OK;
    static const float some_bias = 0.0f;
    DwParams p = dw_shape(B, C, H, W, Ho, Wo, k, stride, pad_lo, act);
    p.bias = has_bias ? &some_bias : nullptr;                      // (dw_choose only asks whether there is one)
    DwChoice c{};
    if (dw_choose(dtype, p, c) != hipSuccess) return CF_OK;
    const int v[16] = {1, c.strip, c.k, c.s, c.th, c.tw, c.Cc, c.nchunk, c.cpp, c.threads, (int)c.lds_bytes, c.ntx, c.nty, (int)c.nwg, Ho, Wo};
    for (int i = 0; i < 16; ++i) out[i] = v[i];
    if (tag) snprintf(tag, (size_t)tag_len, "%s", c.tag);
    return CF_OK;
}

int cf_op_pwconv_ex(int device, int dtype, const float* x, const float* w, const float* bias,
                    const float* residual, float* y, int B, int Cin, int Cout, int H, int W, int act, int layout) {
    if (bad_dtype(dtype) || !x || !w || !y || act < 0 || act > 2) return CF_EINVAL;
    if ((Cin % 8) || (Cout % 8)) return fail("cf_op_pwconv", "Cin and Cout must be multiples of 8");
    if ((layout & ~7) || ((layout & 4) && !residual)) return fail("cf_op_pwconv_ex", "unknown layout bits, or a pixel-block residual without a residual");
    Scope sc(device);
    std::vector<char> packed(pw_packed_bytes(dtype, Cin, Cout));
    pw_pack_weights(dtype, w, Cin, Cout, packed.data());
    PwParams p{};
    p.xblock = layout & 1; p.yblock = (layout >> 1) & 1; p.resblock = (layout >> 2) & 1;
    p.x = p.xblock ? sc.to_blocked(dtype, x, B, Cin, H, W) : sc.to_nhwc(dtype, x, B, Cin, H, W);
    p.wp = sc.up(packed.data(), packed.size());
    p.bias = bias ? sc.in(bias, Cout) : nullptr;
    p.res = !residual ? nullptr : p.resblock ? sc.to_blocked(dtype, residual, B, Cout, H, W) : sc.to_nhwc(dtype, residual, B, Cout, H, W);
    p.y = sc.alloc_nan(p.yblock ? Scope::blocked_bytes(dtype, B, Cout, H, W) : (size_t)B * H * W * Cout * elem_size(dtype));
    p.M = (long long)B * H * W; p.K = Cin; p.N = Cout; p.act = act; p.Ho = H; p.Wo = W;      // the map size picks the kernel (cf_pw.hip)
    sc.run([&] { return launch_pw(sc.s, dtype, p); });
    if (p.yblock) sc.blocked_to_host_nchw(dtype, p.y, y, B, Cout, H, W);
    else sc.to_host_nchw(dtype, p.y, y, B, Cout, H, W);
    return sc.result("cf_op_pwconv");
}
int cf_op_pwconv(int device, int dtype, const float* x, const float* w, const float* bias,
                 const float* residual, float* y, int B, int Cin, int Cout, int H, int W, int act) {
    return cf_op_pwconv_ex(device, dtype, x, w, bias, residual, y, B, Cin, Cout, H, W, act, 0);
}

int cf_op_mbconv(int device, int dtype, const float* x, const float* w_exp, const float* w_dw,
                 const float* w_proj, float* y, int B, int Cin, int hid, int Cout, int H, int W, int k, int stride) {
    if (bad_dtype(dtype) || !x || !w_exp || !w_dw || !w_proj || !y || B < 1) return CF_EINVAL;
    MbGeom g = mb_geometry(dtype, Cin, hid, Cout, k, stride);
    if (!g.ok || hid == Cin) { g_op_error = "shape not covered by the fused MBConv kernel"; return CF_EINVAL; }
    const int pd = k - stride > 0 ? k - stride : 0;
    const int Ho = (H + pd - k) / stride + 1, Wo = (W + pd - k) / stride + 1;
    Scope sc(device);
    std::vector<char> we(g.wexp_bytes), wp(g.wproj_bytes);
    std::vector<float> wd(g.wdw_floats);
    mb_pack_weights(dtype, g, Cin, hid, Cout, k, w_exp, w_dw, w_proj, we.data(), wd.data(), wp.data());
    MbParams p{};
    p.x = sc.to_nhwc(dtype, x, B, Cin, H, W);
    p.y = sc.alloc_nan((size_t)B * Ho * Wo * Cout * elem_size(dtype));
    p.wexp = sc.up(we.data(), we.size()); p.wdw = sc.upv(wd); p.wproj = sc.up(wp.data(), wp.size());
    p.B = B; p.Hin = H; p.Win = W; p.Hout = Ho; p.Wout = Wo; p.Cin = Cin; p.hid = hid; p.Cout = Cout;
    p.k = k; p.s = stride; p.pad_lo = pd / 2; p.residual = (Cin == Cout && stride == 1) ? 1 : 0;
    mb_fill(p, g);
    // (A/B build: the phase cycle sums of mbconv_f32_kernel, MB_F32 [7])
    launch_mbconv_timed(sc, dtype, p, &p.dbg, true, (size_t)1 << 22, 2, [&](float ms, size_t nw, const double* sum) {
        if (nw) fprintf(stderr, "mbconv timing (kind %d): %.1f us; %zu waves, %d chunks each; mean cycles per wave and chunk: wait-top %.0f  expand %.0f  barrier %.0f  dw+project %.0f  (sum %.0f)\n",
                        g.kind, ms * 1e3, nw, g.nq, sum[0] / nw / g.nq, sum[1] / nw / g.nq, sum[2] / nw / g.nq, sum[3] / nw / g.nq, (sum[0] + sum[1] + sum[2] + sum[3]) / nw / g.nq);
    });
    sc.to_host_nchw(dtype, p.y, y, B, Cout, Ho, Wo);
    return sc.result("cf_op_mbconv");
}

// The geometry functions alone (no device, no launch): which family and table row a block shape lands on.
static int pick_out(const MbGeom& g, int out[8]) {
    const int v[8] = {g.ok ? 1 : 0, (int)g.kind, g.HC, g.nq, g.JX, g.NBO, g.HALF, g.KG};
    for (int i = 0; i < 8; ++i) out[i] = g.ok ? v[i] : 0;
    return CF_OK;
}
int cf_op_mbconv_pick(int dtype, int Cin, int hid, int Cout, int k, int stride, int out[8]) {
    if (bad_dtype(dtype) || !out) return CF_EINVAL;
    MbGeom g = mb_geometry(dtype, Cin, hid, Cout, k, stride);
    if (hid == Cin) g.ok = false;
    return pick_out(g, out);
}
int cf_op_expand_dw_pick(int dtype, int Cin, int hid, int k, int stride, int out[8]) {
    if (bad_dtype(dtype) || !out) return CF_EINVAL;
    return pick_out(expdw_geometry(dtype, Cin, hid, k, stride), out);
}

int cf_op_expand_dw(int device, int dtype, const float* x, const float* w_exp, const float* w_dw, float* y,
                    int B, int Cin, int hid, int H, int W, int k, int stride) {
    if (bad_dtype(dtype) || !x || !w_exp || !w_dw || !y || B < 1) return CF_EINVAL;
    MbGeom g = expdw_geometry(dtype, Cin, hid, k, stride);
    if (!g.ok) { g_op_error = "shape / dtype not covered by the expand+depthwise kernel"; return CF_EINVAL; }
    const int pd = k - stride > 0 ? k - stride : 0;
    const int Ho = (H + pd - k) / stride + 1, Wo = (W + pd - k) / stride + 1;
    Scope sc(device);
    std::vector<char> we(g.wexp_bytes);
    std::vector<float> wd(g.wdw_floats);
    mb_pack_weights(dtype, g, Cin, hid, hid, k, w_exp, w_dw, nullptr, we.data(), wd.data(), nullptr);
    MbParams p{};
    p.x = sc.to_nhwc(dtype, x, B, Cin, H, W);
    p.y = sc.alloc_nan((size_t)B * Ho * Wo * hid * elem_size(dtype));
    p.wexp = sc.up(we.data(), we.size()); p.wdw = sc.upv(wd);
    p.B = B; p.Hin = H; p.Win = W; p.Hout = Ho; p.Wout = Wo; p.Cin = Cin; p.hid = hid; p.Cout = hid;
    p.k = k; p.s = stride; p.pad_lo = pd / 2;
    mb_fill(p, g);
    // (A/B build: the phase cycle sums of expdw_f32_kernel, which finds its counters where a projection's weights would be)
    launch_mbconv_timed(sc, dtype, p, &p.wproj, g.kind == XD_F32, (size_t)1 << 20, 3, [&](float ms, size_t nw, const double* sum) {
        const int chunks = g.HALF < g.nq ? g.HALF : g.nq;
        fprintf(stderr, "x5 timing: %.1f us; %zu waves, %d chunks each; mean cycles per wave and chunk: wait-top %.0f  phase1 %.0f  barrier %.0f  phase2 %.0f  (sum %.0f)\n",
                ms * 1e3, nw, chunks, sum[0] / nw / chunks, sum[1] / nw / chunks, sum[2] / nw / chunks, sum[3] / nw / chunks, (sum[0] + sum[1] + sum[2] + sum[3]) / nw / chunks);
    });
    sc.to_host_nchw(dtype, p.y, y, B, hid, Ho, Wo);
    return sc.result("cf_op_expand_dw");
}

int cf_op_ctdet_loss(int device, const float* hm_raw, const float* wh, const float* reg, const float* lm,
                     int B, int h, int w, const float* gt_hm, const uint8_t* reg_mask, const int64_t* ind,
                     const float* wh_t, const float* reg_t, const uint8_t* lm_mask, const int64_t* lm_ind,
                     const float* lm_t, int max_objs, const float* weights4, float* out5) {
    if (!hm_raw || !wh || !reg || !lm || !gt_hm || !reg_mask || !ind || !wh_t || !reg_t || !lm_mask || !lm_ind || !lm_t ||
        !weights4 || !out5 || B < 1 || h < 1 || w < 1 || max_objs < 1) return CF_EINVAL;
    Scope sc(device);
    const size_t hw = (size_t)h * w, bm = (size_t)B * max_objs;
    LossParams p{};
    p.hm_raw = sc.in(hm_raw, B * hw); p.wh = sc.in(wh, B * 2 * hw); p.reg = sc.in(reg, B * 2 * hw); p.lm = sc.in(lm, B * 10 * hw);
    p.gt_hm = sc.in(gt_hm, B * hw);
    p.reg_mask = sc.in(reg_mask, bm); p.ind = (const long long*)sc.in(ind, bm); p.wh_t = sc.in(wh_t, bm * 2); p.reg_t = sc.in(reg_t, bm * 2);
    p.lm_mask = sc.in(lm_mask, bm); p.lm_ind = (const long long*)sc.in(lm_ind, bm); p.lm_t = sc.in(lm_t, bm * 10);
    p.B = B; p.h = h; p.w = w; p.M = max_objs;
    p.hm_w = weights4[0]; p.wh_w = weights4[1]; p.off_w = weights4[2]; p.lm_w = weights4[3];
    const int nblocks = 256;
    double* ws = sc.make<double>(3 * nblocks + 6);
    float* out = sc.out(out5, 5);
    sc.run([&] { return launch_ctdet_loss(sc.s, p, ws, nblocks, out); });
    return sc.result("cf_op_ctdet_loss");
}

int cf_op_encode_targets(int device, const float* boxes, const float* lms, const int32_t* counts, int B, int h, int w,
                         int max_objs, float* hm, float* wh, float* reg, int64_t* ind, uint8_t* reg_mask,
                         float* landmarks, int64_t* lm_ind, uint8_t* lm_mask) {
    if (!boxes || !lms || !counts || !hm || !wh || !reg || !ind || !reg_mask || !landmarks || !lm_ind || !lm_mask ||
        B < 1 || h < 1 || w < 1 || max_objs < 1) return CF_EINVAL;
    for (int b = 0; b < B; ++b) if (counts[b] < 0 || counts[b] > max_objs) return CF_EINVAL;
    Scope sc(device);
    const size_t hw = (size_t)h * w, bm = (size_t)B * max_objs;
    EncodeParams p{};
    p.boxes = sc.in(boxes, bm * 4); p.lms = sc.in(lms, bm * 10); p.counts = sc.in(counts, B);
    p.hm = sc.out(hm, B * hw); p.wh = sc.out(wh, bm * 2); p.reg = sc.out(reg, bm * 2);
    p.ind = (long long*)sc.out(ind, bm); p.reg_mask = sc.out(reg_mask, bm);
    p.landmarks = sc.out(landmarks, bm * 10); p.lm_ind = (long long*)sc.out(lm_ind, bm); p.lm_mask = sc.out(lm_mask, bm);
    p.B = B; p.h = h; p.w = w; p.M = max_objs;
    sc.run([&] { return launch_encode_targets(sc.s, p); });
    return sc.result("cf_op_encode_targets");
}

int cf_op_stem(int device, int dtype, const void* x, int in_format, const float* w, float* y, int B, int H, int W) {
    if (bad_dtype(dtype) || !x || !w || !y || (H % 2) || (W % 2)) return CF_EINVAL;
    if (in_format != CF_IN_U8_HWC_BGR && in_format != CF_IN_F32_NCHW) return CF_EINVAL;
    Scope sc(device);
    std::vector<char> wp(stem_packed_bytes(dtype));
    stem_pack_weights(dtype, w, wp.data());
    StemParams p{};
    p.x = sc.up(x, (size_t)B * 3 * H * W * (in_format == CF_IN_U8_HWC_BGR ? 1 : 4));
    p.in_format = in_format; p.w = sc.up(wp.data(), wp.size());
    p.y = sc.alloc((size_t)B * (H / 2) * (W / 2) * 32 * elem_size(dtype));
    p.B = B; p.H = H; p.W = W;
    sc.run([&] { return launch_stem(sc.s, dtype, p); });
    sc.to_host_nchw(dtype, p.y, y, B, 32, H / 2, W / 2);
    return sc.result("cf_op_stem");
}

int cf_op_idaup(int device, int dtype, const float* lo, const float* skip, const float* w_up,
                const float* bn_up, const float* w_cv, const float* bn_cv, float eps, float* y,
                int B, int C, int Cs, int h, int w) {
    if (bad_dtype(dtype) || !lo || !skip || !w_up || !bn_up || !w_cv || !bn_cv || !y || (C % 8) || (Cs % 8)) return CF_EINVAL;
    Scope sc(device);
    std::vector<double> s1, h1, s2, h2;
    fold(bn_cv, C, eps, s1, h1);
    fold(bn_up, C, eps, s2, h2);
    std::vector<float> wf((size_t)C * Cs), bias(C), uw(4 * C), ub(C);
    for (int n = 0; n < C; ++n) {
        for (int k = 0; k < Cs; ++k) wf[(size_t)n * Cs + k] = (float)((double)w_cv[(size_t)n * Cs + k] * s1[n]);
        bias[n] = (float)h1[n];
        for (int t = 0; t < 4; ++t) uw[(size_t)t * C + n] = (float)((double)w_up[n * 4 + t] * s2[n]);
        ub[n] = (float)h2[n];
    }
    std::vector<char> packed(pw_packed_bytes(dtype, Cs, C));
    pw_pack_weights(dtype, wf.data(), Cs, C, packed.data());
    const int Ho = 2 * h, Wo = 2 * w;
    PwParams p{};
    p.x = sc.to_nhwc(dtype, skip, B, Cs, Ho, Wo);
    p.low = sc.to_nhwc(dtype, lo, B, C, h, w);
    p.wp = sc.up(packed.data(), packed.size());
    p.bias = sc.upv(bias); p.upw = sc.upv(uw); p.upb = sc.upv(ub);
    p.y = sc.alloc((size_t)B * Ho * Wo * C * elem_size(dtype));
    p.M = (long long)B * Ho * Wo; p.K = Cs; p.N = C; p.act = 2; p.Ho = Ho; p.Wo = Wo;
    sc.run([&] { return launch_pw(sc.s, dtype, p); });
    sc.to_host_nchw(dtype, p.y, y, B, C, Ho, Wo);
    return sc.result("cf_op_idaup");
}

int cf_op_heads(int device, int dtype, const float* x, const float* w0, const float* b0,
                const float* w1, const float* b1, float* out, int B, int h, int w, int collapse) {
    if (bad_dtype(dtype) || !x || !w0 || !b0 || !w1 || !b1 || !out) return CF_EINVAL;
    Scope sc(device);
    std::vector<char> packed(head_packed_bytes(dtype, collapse ? 1 : 0));
    std::vector<float> b0h(96), w1d(96 * 16), b1h(16);
    head_pack_weights(dtype, collapse ? 1 : 0, w0, b0, w1, b1, packed.data(), b0h.data(), w1d.data(), b1h.data());
    HeadParams p{};
    p.x = sc.to_nhwc(dtype, x, B, 24, h, w);
    p.w0p = sc.up(packed.data(), packed.size());
    p.b0 = sc.upv(b0h); p.w1d = sc.upv(w1d); p.b1 = sc.upv(b1h);
    const size_t HW = (size_t)h * w;
    std::vector<float> rec((size_t)B * HW * 16);
    p.heads = sc.out(rec.data(), rec.size());
    p.B = B; p.h = h; p.w = w; p.collapsed = collapse ? 1 : 0;
    sc.run([&] { return launch_heads(sc.s, dtype, p); });
    int r = sc.result("cf_op_heads");
    if (r) return r;
    for (int b = 0; b < B; ++b)
        for (size_t i = 0; i < HW; ++i) {
            const float* rr = &rec[((size_t)b * HW + i) * 16];
            out[((size_t)b * 15 + 0) * HW + i] = rr[15];                      // raw hm logit
            for (int c = 1; c < 15; ++c) out[((size_t)b * 15 + c) * HW + i] = rr[c];
        }
    return CF_OK;
}

// ShuffleV2Block.forward, eval mode (model/blocks.py:47-62).  BatchNorm is folded here (float64) into the conv
// weights + an fp32 bias; the channel shuffle is ADDRESSING, not data movement on the host: the first 1x1 conv of
// branch_main reads the odd input channels through a zero-interleaved weight matrix over all 2*inp channels (exact:
// the even channels meet zero weights), the pass-through half is copied by a strided-channel kernel straight into
// channels [0, inp) of the block output, and both final 1x1 convs write their slice of the output rows
// (PwParams::ldy / yoff) -- the torch.cat of the reference never materialises.
int cf_op_shufflev2(int device, int dtype, const float* x, float* y, int B, int inp, int oup, int mid, int H, int W,
                    int ksize, int stride, const float* m_w0, const float* m_bn1, const float* m_wdw, const float* m_bn4,
                    const float* m_w5, const float* m_bn6, const float* p_wdw, const float* p_bn1, const float* p_w2,
                    const float* p_bn3) {
    const int outputs = oup - inp;
    if (bad_dtype(dtype) || !x || !y || B < 1 || (ksize != 3 && ksize != 5) || (stride != 1 && stride != 2) || outputs < 8 ||
        (inp % 8) || (mid % 8) || (outputs % 8) || !m_w0 || !m_bn1 || !m_wdw || !m_bn4 || !m_w5 || !m_bn6) return CF_EINVAL;
    if (stride == 2 && (!p_wdw || !p_bn1 || !p_w2 || !p_bn3)) return CF_EINVAL;
    const int Cin = stride == 1 ? 2 * inp : inp, pad = ksize / 2;
    const int Ho = (H + 2 * pad - ksize) / stride + 1, Wo = (W + 2 * pad - ksize) / stride + 1;
    const float eps = 1e-5f;                                             // nn.BatchNorm2d default (blocks.py:23,29,32)
    Scope sc(device);
    void* xd = sc.to_nhwc(dtype, x, B, Cin, H, W);
    void* out = sc.alloc((size_t)B * Ho * Wo * oup * elem_size(dtype));
    const long long Min = (long long)B * H * W, Mout = (long long)B * Ho * Wo;

    auto pw = [&](const void* src, long long M, int K, int N, const float* w /*[N][Kw]*/, int Kw, bool interleave, const float* bn,
                  void* dst, int ldy, int yoff) {
        std::vector<double> s1, h1;
        fold(bn, N, eps, s1, h1);
        std::vector<float> wf((size_t)N * K, 0.0f), bias(N);
        for (int n = 0; n < N; ++n) {
            for (int k = 0; k < Kw; ++k) wf[(size_t)n * K + (interleave ? 2 * k + 1 : k)] = (float)((double)w[(size_t)n * Kw + k] * s1[n]);
            bias[n] = (float)h1[n];
        }
        std::vector<char> packed(pw_packed_bytes(dtype, K, N));
        pw_pack_weights(dtype, wf.data(), K, N, packed.data());
        PwParams p{};
        p.x = src; p.wp = sc.up(packed.data(), packed.size()); p.bias = sc.upv(bias); p.y = dst;
        p.M = M; p.K = K; p.N = N; p.act = 2; p.ldy = ldy; p.yoff = yoff;
        sc.run([&] { return launch_pw(sc.s, dtype, p); });
    };
    auto dw = [&](const void* src, int C, const float* w /*[C][1][k][k]*/, const float* bn) -> void* {
        std::vector<double> s1, h1;
        fold(bn, C, eps, s1, h1);
        std::vector<float> wf((size_t)C * ksize * ksize), wp((size_t)C * ksize * ksize), bias(C);
        for (int c = 0; c < C; ++c) {
            for (int t = 0; t < ksize * ksize; ++t) wf[(size_t)c * ksize * ksize + t] = (float)((double)w[(size_t)c * ksize * ksize + t] * s1[c]);
            bias[c] = (float)h1[c];
        }
        dw_pack_weights(wf.data(), C, ksize, wp.data());
        DwParams p{};
        p.x = src; p.w = sc.upv(wp); p.bias = sc.upv(bias);
        p.y = sc.alloc((size_t)Mout * C * elem_size(dtype));
        p.B = B; p.C = C; p.H = H; p.W = W; p.Ho = Ho; p.Wo = Wo; p.k = ksize; p.s = stride; p.pad_lo = pad; p.act = 0;
        sc.run([&] { return launch_dw(sc.s, dtype, p); });
        return p.y;
    };

    // branch_main (:20-34): pw + BN + ReLU -> dw + BN -> pw + BN + ReLU, into channels [inp, oup)
    void* t1 = sc.alloc((size_t)Min * mid * elem_size(dtype));
    pw(xd, Min, Cin, mid, m_w0, inp, stride == 1, m_bn1, t1, 0, 0);
    void* t2 = dw(t1, mid, m_wdw, m_bn4);
    pw(t2, Mout, mid, outputs, m_w5, mid, false, m_bn6, out, oup, inp);
    if (stride == 1) {
        // x_proj = the even channels (:56-62), passed through into channels [0, inp)
        sc.run([&] { return launch_shuffle_copy(sc.s, dtype, xd, out, Min, inp, 0, oup, 0); });
    } else {
        // branch_proj (:36-45): dw + BN -> pw + BN + ReLU, into channels [0, inp)
        void* p1 = dw(xd, inp, p_wdw, p_bn1);
        pw(p1, Mout, inp, inp, p_w2, inp, false, p_bn3, out, oup, 0);
    }
    sc.to_host_nchw(dtype, out, y, B, oup, Ho, Wo);
    return sc.result("cf_op_shufflev2");
}

int cf_op_ctdet_decode(int device, const float* heat, const float* wh, const float* reg, const float* lm,
                       int B, int h, int w, int K, float* dets, float* lms, int64_t* inds) {
    if (!heat || !wh || !dets || B < 1 || K < 1 || (long long)K > (long long)h * w) return CF_EINVAL;
    Scope sc(device);
    std::vector<float> rec = make_records(heat, wh, reg, lm, B, h, w);
    TopkParams p{};
    p.heads = sc.upv(rec);
    p.scratch = sc.make<unsigned long long>((size_t)B * h * w);
    p.count = sc.make<int>((size_t)B * kTopkCountStride);               // zero-initialised by Scope::alloc
    if (K > 1024) { p.big_stride = topk_big_stride(K); p.big = sc.make<unsigned long long>((size_t)B * p.big_stride); }
    p.B = B; p.h = h; p.w = w; p.K = K; p.use_reg = reg ? 1 : 0;
    p.dets = sc.out(dets, (size_t)B * K * 6);
    p.lms = (lms && lm) ? sc.out(lms, (size_t)B * K * 10) : nullptr;
    p.inds = inds ? (long long*)sc.out(inds, (size_t)B * K) : nullptr;
    sc.run([&] { return launch_peak_topk(sc.s, p); });
    return sc.result("cf_op_ctdet_decode");
}

static int run_threshold(Scope& sc, int mode, const float* d_heads, int B, int h, int w, int img_h, int img_w,
                         float score_thresh, float nms_thresh, int cap, int max_out,
                         float* dets, float* lms, int32_t* counts, int* overflow_out) {
    const size_t words = (cap + 63) / 64;
    ThreshParams p{};
    p.heads = d_heads; p.B = B; p.h = h; p.w = w; p.img_h = img_h; p.img_w = img_w;
    p.score_thresh = score_thresh; p.nms_thresh = nms_thresh; p.cap = cap; p.mode = mode;
    p.cand = sc.make<float>((size_t)B * cap * 16);
    p.cand_count = sc.make<int>(B);
    p.order = sc.make<int>((size_t)B * cap);
    p.mask = sc.make<unsigned long long>((size_t)B * cap * words);
    p.max_out = max_out;
    p.dets = sc.out(dets, (size_t)B * max_out * 5);
    p.lms = lms ? sc.out(lms, (size_t)B * max_out * 10) : nullptr;
    p.counts = sc.out(counts, B);
    p.overflow = sc.out(overflow_out, 1);
    sc.run([&] { return launch_decode_threshold(sc.s, p); });
    return sc.result("decode_threshold");
}

int cf_op_decode_threshold(int device, const float* hm, const float* wh, const float* lm,
                           int B, int h, int w, int img_h, int img_w, float score_thresh,
                           float nms_thresh, int max_out, float* dets, float* lms, int32_t* counts) {
    return cf_op_decode_threshold_ex(device, 0, hm, wh, nullptr, lm, B, h, w, img_h, img_w, score_thresh, nms_thresh,
                                     max_out, dets, lms, counts);
}

int cf_op_decode_threshold_ex(int device, int mode, const float* hm, const float* wh, const float* reg, const float* lm,
                              int B, int h, int w, int img_h, int img_w, float score_thresh,
                              float nms_thresh, int max_out, float* dets, float* lms, int32_t* counts) {
    if (!hm || !wh || !dets || !counts || B < 1 || max_out < 1 || (mode != 0 && mode != 1) || (mode == 1 && !reg)) return CF_EINVAL;
    Scope sc(device);
    std::vector<float> rec = make_records(hm, wh, reg, lm, B, h, w);
    const float* d_heads = sc.upv(rec);
    const int HW = h * w;
    int cap = HW < 4096 ? (HW + 63) / 64 * 64 : 4096;
    for (int attempt = 0; attempt < 2; ++attempt) {            // grow to the largest candidate count and rerun (see cf_decode_threshold_ex)
        int overflow = 0;
        int r = run_threshold(sc, mode, d_heads, B, h, w, img_h, img_w, score_thresh, nms_thresh, cap, max_out, dets, lms, counts, &overflow);
        if (r) return r;
        if (overflow <= cap) return CF_OK;
        cap = ((overflow < HW ? overflow : HW) + 63) / 64 * 64;
    }
    g_op_error = "candidate capacity exceeded";
    return CF_EOVERFLOW;
}

int cf_op_ctdet_post_process(int device, float* dets, const float* centers, const float* scales, int B, int K, int dim,
                             int out_w, int out_h) {
    if (!dets || !centers || !scales || B < 1 || K < 1 || dim < 4) return CF_EINVAL;
    Scope sc(device);
    std::vector<double> t((size_t)B * 6);
    for (int b = 0; b < B; ++b) cf_affine_from_center_scale(centers[2 * b], centers[2 * b + 1], scales[2 * b], out_w, out_h, &t[(size_t)b * 6]);
    float* d = sc.inout(dets, (size_t)B * K * dim);
    double* dt = sc.upv(t);
    sc.run([&] { return launch_affine_boxes(sc.s, d, dt, B, K, dim); });
    return sc.result("cf_op_ctdet_post_process");
}

int cf_op_nms(int device, const float* boxes, const float* scores, int n, float nms_thresh, int32_t* keep, int32_t* n_keep) {
    // CenterFace.nms alone: feed the candidates through the D1 kernels' rank/mask/sweep stages by
    // presenting them as pre-collected candidates.
    if (!boxes || !scores || !keep || !n_keep || n < 0) return CF_EINVAL;
    if (n == 0) { *n_keep = 0; return CF_OK; }
    Scope sc(device);
    const int cap = (n + 63) / 64 * 64;
    const size_t words = cap / 64;
    std::vector<float> cand((size_t)cap * 16, 0.0f);
    for (int i = 0; i < n; ++i) {
        for (int j = 0; j < 4; ++j) cand[(size_t)i * 16 + j] = boxes[i * 4 + j];
        cand[(size_t)i * 16 + 4] = scores[i];
        cand[(size_t)i * 16 + 5] = (float)i;           // carried through as "landmark 0" = original index
    }
    ThreshParams p{};
    p.B = 1; p.cap = cap; p.nms_thresh = nms_thresh;
    p.cand = sc.upv(cand);
    p.cand_count = sc.in(&n, 1);
    p.order = sc.make<int>(cap);
    p.mask = sc.make<unsigned long long>((size_t)cap * words);
    p.max_out = n;
    std::vector<float> l((size_t)n * 10);
    int cnt = 0;
    p.dets = sc.make<float>((size_t)n * 5);
    p.lms = sc.out(l.data(), l.size());
    p.counts = sc.out(&cnt, 1);
    p.overflow = sc.make<int>(1);
    sc.run([&] { return launch_nms_stages(sc.s, p); });
    int r = sc.result("cf_op_nms");
    if (r) return r;
    for (int i = 0; i < cnt; ++i) keep[i] = (int32_t)l[(size_t)i * 10];
    *n_keep = cnt;
    return CF_OK;
}

// bbox_overlap (eval_widerface.py:48-74) and the match counts of evaluate (:195-206) for n_img images at once: boxes / query are
// the concatenated rows, box_off / query_off [n_img + 1] the first row of each image.  overlaps (optional): the dense [N_i][K_i]
// float64 matrices back to back; counts (optional) [n_img][2].
int cf_op_box_match(int device, int n_img, const float* boxes, int box_stride, const int32_t* box_off, const float* query, int query_stride,
                    const int32_t* query_off, float thresh, double* overlaps, int32_t* counts) {
    if (n_img < 0 || !box_off || !query_off || box_stride < 4 || query_stride < 4) return CF_EINVAL;
    if (n_img == 0) return CF_OK;
    const int NB = box_off[n_img], NQ = query_off[n_img];
    if (box_off[0] != 0 || query_off[0] != 0 || (NB > 0 && !boxes) || (NQ > 0 && !query)) return CF_EINVAL;
    std::vector<long long> ooff(n_img + 1, 0);
    for (int i = 0; i < n_img; ++i) {
        const int N = box_off[i + 1] - box_off[i], K = query_off[i + 1] - query_off[i];
        if (N < 0 || K < 0) return CF_EINVAL;
        ooff[i + 1] = ooff[i] + (long long)N * K;
    }
    Scope sc(device);
    OverlapParams p{};
    p.n_img = n_img; p.box_stride = box_stride; p.query_stride = query_stride; p.thresh = thresh;
    float dummy[4] = {0, 0, 0, 0};
    p.boxes = sc.in(NB ? boxes : dummy, NB ? (size_t)NB * box_stride : 4);
    p.query = sc.in(NQ ? query : dummy, NQ ? (size_t)NQ * query_stride : 4);
    p.box_off = sc.in(box_off, (size_t)n_img + 1);
    p.query_off = sc.in(query_off, (size_t)n_img + 1);
    if (overlaps && ooff[n_img] > 0) {
        p.overlaps = sc.out(overlaps, (size_t)ooff[n_img]);
        p.overlaps_off = sc.upv(ooff);
    }
    if (counts) p.counts = sc.out(counts, (size_t)n_img * 2);
    sc.run([&] { return launch_box_match(sc.s, p); });
    return sc.result("cf_op_box_match");
}

// The conversion kernel of cf_forward_yuv on dense host frames [B][h*3/2][w] -> bgr [B][H][W][3] ((H, W) != (h, w): convert + resize).
int cf_op_yuv_to_bgr(int device, int yuv_format, const uint8_t* frames, uint8_t* bgr, int B, int h, int w, int H, int W) {
    if (!frames || !bgr || B < 1 || yuv_format < CF_YUV_NV12 || yuv_format > CF_YUV_YV12 || h < 2 || w < 2 || (h & 1) || (w & 1) ||
        H < 1 || W < 2 || (W & 1))
        return fail("cf_op_yuv_to_bgr", "null buffer, B < 1, unknown format, or h / w / W not even and at least 2");
    const bool il = yuv_format == CF_YUV_NV12 || yuv_format == CF_YUV_NV21;
    const int cw = il ? w : w / 2;
    const size_t ybytes = (size_t)h * w, cbytes = (size_t)(h / 2) * cw, one = ybytes + (il ? cbytes : 2 * cbytes);
    Scope sc(device);
    const uint8_t* src = sc.in(frames, one * B);
    uint8_t* out = sc.out(bgr, (size_t)B * H * W * 3);
    std::vector<const void*> planes((size_t)3 * B);
    for (int b = 0; b < B && src; ++b) {
        const uint8_t* f = src + b * one;
        planes[3 * b] = f; planes[3 * b + 1] = f + ybytes; planes[3 * b + 2] = il ? nullptr : f + ybytes + cbytes;
    }
    sc.run([&] { return launch_yuv_to_bgr(sc.s, yuv_format, planes.data(), B, h, w, w, cw, out, H, W); });
    return sc.result("cf_op_yuv_to_bgr");
}

int cf_op_align_faces(int device, const uint8_t* imgs, int B, int h, int w, const float* lms, const int32_t* counts,
                      const cf_align_opts* o, void* chips, double* matrices) {
    if (!imgs || !counts || !o || !chips || B < 1 || h < 1 || w < 2)
        return fail("cf_op_align_faces", "null images, counts, options or chips, B < 1, h < 1 or w < 2");
    AlignParams p{};
    const char* why = align_params_set(p, o->size, o->format, o->rgb, o->mean, o->scale, o->tmpl, o->max_per_image);
    long long N = 0;
    if (!why) why = count_rows(counts, B, INT_MAX, "negative count", nullptr, &N);
    if (!why && N > 0 && !lms) why = "null landmarks";
    if (!why && N > (1 << 24)) why = "more than 2^24 faces";
    if (why) return fail("cf_op_align_faces", why);
    if (N == 0) return CF_OK;
    Scope sc(device);
    const size_t img_bytes = (size_t)B * h * w * 3;
    p.img = sc.in(imgs, img_bytes); p.img_dwords = (img_bytes + 3) / 4;      // (Scope pads every allocation)
    p.B = B; p.H = h; p.W = w;
    align_rows(sc, p, lms, counts, B, N, o, chips, matrices);
    sc.run([&] { return launch_align_faces(sc.s, p); });
    return sc.result("cf_op_align_faces");
}

// The kernel of cf_align_faces_frame on host frames.
int cf_op_align_frame(int device, int format, const cf_yuv_planes* host_frames, int B, int h, int w, int pitch0, int pitch1,
                      const float* lms, const int32_t* counts, const cf_align_opts* o, void* chips, double* matrices) {
    static_assert(sizeof(cf_yuv_planes) == 3 * sizeof(void*), "cf_yuv_planes is a table of three addresses");
    const void* const* hp = reinterpret_cast<const void* const*>(host_frames);
    AlignFrameParams p{};
    const char* why = nullptr;
    if (!o || !chips || !counts) why = "null options, chips or counts";
    if (!why) why = align_frame_check(p, o->size, o->format, o->rgb, o->mean, o->scale, o->tmpl, o->max_per_image, format, hp, 0, B, h, w, pitch0, pitch1);
    if (!why && ((pitch0 & 3) || (format != CF_FRAME_BGR && (pitch1 & 3)))) why = "pitches must be multiples of 4 (the planes are read on the device as they are)";
    long long N = 0;
    if (!why) why = count_rows(counts, B, INT_MAX, "negative count", nullptr, &N);
    if (!why && N > 0 && !lms) why = "null landmarks";
    if (!why && N > (1 << 24)) why = "more than 2^24 faces";
    if (why) return fail("cf_op_align_frame", why);
    if (N == 0) return CF_OK;
    Scope sc(device);
    const std::vector<const void*> dev = up_planes(sc, format, hp, B, h, pitch0, pitch1);
    p.planes = dev.data(); p.sx = 1.0; p.sy = 1.0;
    align_rows(sc, p.a, lms, counts, B, N, o, chips, matrices);
    sc.run([&] { return launch_align_frame(sc.s, p); });
    return sc.result("cf_op_align_frame");
}

// The kernels of cf_redact_faces on host frames (in place).
int cf_op_redact(int device, const cf_redact_opts* o, int format, const cf_planes_rw* frames, int B, int h, int w, int pitch0, int pitch1,
                 const float* boxes, const int32_t* counts, int H, int W) {
    if (!o) return fail("cf_op_redact", "null options");
    const char* why = redact_check(format, o->mode, o->shape, o->cell, o->scale, B, h, w, pitch0, pitch1);
    return op_on_faces("cf_op_redact", why, device, FrameGeo{format, B, h, w, pitch0, pitch1}, frames, boxes, counts, H, W,
                       [&](Scope& sc, const FrameGeo& g, const void* const* planes, const FaceList& f) {
        RedactParams p{};
        p.g = g; p.f = f; p.planes = planes; p.mode = o->mode; p.shape = o->shape; p.cell = o->cell; p.scale = o->scale;
        p.fill[0] = o->fill[0]; p.fill[1] = o->fill[1]; p.fill[2] = o->fill[2];
        if (o->mode == CF_REDACT_MOSAIC) p.cells = sc.make<uint32_t>(redact_cells(B, h, w, o->cell));
        sc.run([&] { return launch_redact_faces(sc.s, p); });
    });
}

// The kernels of cf_blur_faces on host frames (in place).
int cf_op_blur(int device, const cf_blur_opts* o, int format, const cf_planes_rw* frames, int B, int h, int w, int pitch0, int pitch1,
               const float* boxes, const int32_t* counts, int H, int W) {
    if (!o) return fail("cf_op_blur", "null options");
    const char* why = blur_check(format, o->shape, o->radius, o->scale, B, h, w, pitch0, pitch1);
    return op_on_faces("cf_op_blur", why, device, FrameGeo{format, B, h, w, pitch0, pitch1}, frames, boxes, counts, H, W,
                       [&](Scope& sc, const FrameGeo& g, const void* const* planes, const FaceList& f) {
        BlurParams p{};
        p.g = g; p.f = f; p.planes = planes; p.shape = o->shape; p.radius = o->radius; p.scale = o->scale;
        p.scratch = (uint8_t*)sc.alloc(blur_scratch_bytes(format, B, h, w));
        sc.run([&] { return launch_blur_faces(sc.s, p); });
    });
}

// The kernels of cf_draw_faces on host frames (in place).  The packed rows are spread to [B][max count] like op_on_faces' boxes.
int cf_op_draw(int device, const cf_draw_opts* o, int format, const cf_planes_rw* frames, int B, int h, int w, int pitch0, int pitch1,
               const float* boxes, const float* scores, const float* lms, const int32_t* info, const int32_t* counts, int H, int W) {
    if (!o) return fail("cf_op_draw", "null options");
    const void* const* host_planes = reinterpret_cast<const void* const*>(frames);
    const char* why = draw_check(o, format, B, h, w, pitch0, pitch1);
    if (!why) why = redact_check_planes(format, host_planes, B, 0, pitch0, pitch1);
    if (!why && (!counts || H < 1 || W < 1)) why = "null counts, or H / W below 1";
    if (!why && (o->what & CF_DRAW_LANDMARKS) && !lms) why = "CF_DRAW_LANDMARKS without landmark rows";
    if (!why && o->label == CF_DRAW_LABEL_ID && !info) why = "CF_DRAW_LABEL_ID without info rows";
    int rows = 1;
    long long N = 0;
    if (!why) why = count_rows(counts, B, 1 << 20, "a count is negative or above 2^20", &rows, &N);
    if (!why && N > 0 && (!boxes || !scores)) why = "null boxes or scores";
    if (why) return fail("cf_op_draw", why);
    if (N == 0) return CF_OK;
    const std::vector<float> sb = spread(boxes, counts, B, rows, 4), ss = spread(scores, counts, B, rows, 1), sl = spread(lms, counts, B, rows, 10);
    const std::vector<int32_t> si = spread(info, counts, B, rows, 3);
    Scope sc(device);
    DrawParams p{};
    p.o = *o;
    p.r = DrawRows{sc.upv(sb), sc.upv(ss), 1, lms ? sc.upv(sl) : nullptr, info ? sc.upv(si) : nullptr, sc.in(counts, B), rows, rows, H, W};
    const Staged fr = sc.stage(format, host_planes, B, h, w, pitch0, pitch1);
    p.g = fr.geo(B); p.planes = fr.planes();
    p.recs = (DrawRec*)sc.alloc(draw_scratch_bytes(B, rows));
    sc.run([&] { return launch_draw_faces(sc.s, p); });
    sc.unstage(fr);
    return sc.result("cf_op_draw");
}

int cf_tile_grid(int h, int w, int tile_h, int tile_w, int overlap, int with_full, cf_tile_rect* rects, int cap, int* n) {
    const int r = tile_grid(h, w, tile_h, tile_w, overlap, with_full, rects, cap, n);
    if (r) g_op_error = "cf_tile_grid: h, w, tile_h, tile_w, overlap must be even, the sizes at least 2, 0 <= overlap < min(tile_h, tile_w); n not null";
    return r;
}

// The cutter of cf_forward_tiles on host frames.
int cf_op_cut_tiles(int device, int format, const cf_yuv_planes* host_frames, int Bf, int h, int w, int pitch0, int pitch1,
                    const cf_tile_rect* rects, int T, int H, int W, uint8_t* tiles) {
    static_assert(sizeof(cf_yuv_planes) == 3 * sizeof(void*), "cf_yuv_planes is a table of three addresses");
    std::string why;
    const char* bad = tiles_check(why, format, Bf, h, w, pitch0, pitch1, rects, T, H, W);
    if (!bad) bad = redact_check_planes(format, reinterpret_cast<const void* const*>(host_frames), Bf, 0, pitch0, pitch1);
    if (!bad && !tiles) bad = "null output";
    if (!bad && (long long)Bf * T * H * W * 3 > INT_MAX) bad = "more than 2^31 output bytes";
    if (bad) return fail("cf_op_cut_tiles", bad);
    Scope sc(device);
    const std::vector<const void*> dev = up_planes(sc, format, reinterpret_cast<const void* const*>(host_frames), Bf, h, pitch0, pitch1);
    const cf_tile_rect* drects = sc.in(rects, T);
    uint8_t* out = sc.out(tiles, (size_t)Bf * T * H * W * 3);
    sc.run([&] { return launch_cut_tiles(sc.s, format, dev.data(), Bf, pitch0, pitch1, drects, T, out, H, W); });
    return sc.result("cf_op_cut_tiles");
}

// The merges on host tables.  merge_opts_check: the argument checks the three families share, in their order (nullptr: go on with the
// geometry).  op_merge: the out-of-memory guard, the staging and the launch; p carries the kind, V, Bf, the sizes and the turn, table the
// kind's host table (rectangles, views, or the blob of `pack`), n_img = the number of decoded images, what = the guard's words for V.
static const char* merge_opts_check(const cf_merge_opts* o, const float* dets_net, const float* scores, const float* lms_net, const int32_t* counts, int rows,
                                    int max_out, int H, int W, const float* dets, const float* lms, const int32_t* out_counts, const int32_t* flags) {
    if (!o || !dets_net || !scores || !lms_net || !counts || !dets || !lms || !out_counts || !flags) return "null argument";
    if (o->metric != CF_MERGE_IOU && o->metric != CF_MERGE_IOS) return "unknown metric (0 = CF_MERGE_IOU, 1 = CF_MERGE_IOS)";
    if (!(o->thresh >= 0.f) || !(o->edge >= 0.f) || !std::isfinite(o->thresh) || !std::isfinite(o->edge)) return "thresh and edge must be finite and not negative";
    if (rows < 1 || max_out < 1 || H < 1 || W < 1) return "rows, max_out, H and W must be at least 1";
    return nullptr;
}
static int op_merge(const char* who, int device, MergeParams p, const void* table, size_t table_bytes, const PackHost* pack, size_t n_img, const char* what, const cf_merge_opts* o,
                    const float* dets_net, const float* scores, const float* lms_net, const int32_t* counts, int rows, int max_out, float* dets, float* lms,
                    int32_t* out_counts, int32_t* flags) {
    const int Bf = p.Bf, V = p.V;
    if ((long long)V * rows > (1 << 24) || merge_mask_bytes(Bf, V, rows) > kMergeMaskLimit) {
        g_op_error = std::string(who) + ": the suppression bits of Bf x (" + what + " * rows) candidates exceed 256 MiB";
        return CF_ENOMEM;
    }
    Scope sc(device);
    const size_t n = n_img * rows, cap = (size_t)V * rows, mo = (size_t)Bf * max_out;
    const unsigned char* tab = sc.in((const unsigned char*)table, table_bytes);
    if (p.kind == MERGE_TILES) p.rects = (const cf_tile_rect*)tab;
    else if (p.kind == MERGE_VIEWS) p.views = (const cf_view*)tab;
    else p.pack = pack_dev(*pack, tab);
    p.dets_net = sc.in(dets_net, n * 4);
    p.scores = sc.in(scores, n); p.score_stride = 1;
    p.lms_net = sc.in(lms_net, n * 10);
    p.counts = sc.in(counts, n_img); p.rows = rows;
    p.metric = o->metric; p.thresh = o->thresh; p.edge = o->edge;
    p.cand = sc.make<float>(Bf * cap * 16); p.cand_count = sc.make<int>(Bf);
    p.order = sc.make<int>(Bf * cap); p.mask = (unsigned long long*)sc.alloc(merge_mask_bytes(Bf, V, rows));
    p.max_out = max_out;
    p.dets = sc.inout(dets, mo * 5); p.lms = sc.inout(lms, mo * 10);
    p.corners = sc.make<float>(mo * 4);
    p.out_counts = sc.out(out_counts, Bf); p.flags = sc.out(flags, Bf);
    sc.run([&] { return launch_merge(sc.s, p); });
    return sc.result(who);
}

int cf_op_merge_tiles(int device, const cf_merge_opts* o, const cf_tile_rect* rects, int T, int Bf, int h, int w, int H, int W,
                      const float* dets_net, const float* scores, const float* lms_net, const int32_t* counts, int rows, int max_out,
                      float* dets, float* lms, int32_t* out_counts, int32_t* flags) {
    std::string why;
    const char* bad = merge_opts_check(o, dets_net, scores, lms_net, counts, rows, max_out, H, W, dets, lms, out_counts, flags);
    if (!bad) bad = tiles_check(why, CF_FRAME_BGR, Bf, h, w, 3 * w, 0, rects, T, H, 4);      // the geometry part: frame and rectangles
    if (bad) return fail("cf_op_merge_tiles", bad);
    MergeParams p{};
    p.kind = MERGE_TILES; p.V = T; p.Bf = Bf; p.h = h; p.w = w; p.H = H; p.W = W;
    return op_merge("cf_op_merge_tiles", device, p, rects, (size_t)T * sizeof(cf_tile_rect), nullptr, (size_t)Bf * T, "T", o, dets_net, scores,
                    lms_net, counts, rows, max_out, dets, lms, out_counts, flags);
}

int cf_view_layout(const cf_view_opts* o, int h, int w, int H, int W, cf_view* views, int cap, int* n) {
    const int r = view_layout(o, h, w, H, W, views, cap, n);
    if (r) g_op_error = "cf_view_layout: anchor 0 or 1, 0 <= n_levels <= 8, scales in 1..1000 per mille, h and w in 2..8192, H and W at least 1, tiles as cf_tile_grid "
                        "takes them (or tile_h = tile_w = 0), and at least one view in the result; opts and n not null";
    return r;
}

// The cutter of cf_forward_views on host frames.
int cf_op_views(int device, int format, const cf_yuv_planes* host_frames, int Bf, int h, int w, int pitch0, int pitch1, const cf_view* views,
                int V, const uint8_t* fill, int H, int W, uint8_t* canvases) {
    std::string why;
    const char* bad = views_check(why, format, Bf, h, w, pitch0, pitch1, views, V, H, W);
    if (!bad) bad = redact_check_planes(format, reinterpret_cast<const void* const*>(host_frames), Bf, 0, pitch0, pitch1);
    if (!bad && (!fill || !canvases)) bad = "null fill or output";
    if (!bad && (long long)Bf * V * H * W * 3 > INT_MAX) bad = "more than 2^31 output bytes";
    if (bad) return fail("cf_op_views", bad);
    Scope sc(device);
    const std::vector<const void*> dev = up_planes(sc, format, reinterpret_cast<const void* const*>(host_frames), Bf, h, pitch0, pitch1);
    const cf_view* dviews = sc.in(views, V);
    uint8_t* out = sc.out(canvases, (size_t)Bf * V * H * W * 3);
    sc.run([&] { return launch_cut_views(sc.s, format, dev.data(), Bf, pitch0, pitch1, dviews, V, fill, out, H, W); });
    return sc.result("cf_op_views");
}

int cf_op_merge_views(int device, const cf_merge_opts* o, const cf_view* views, int V, int Bf, int h, int w, int H, int W,
                      const float* dets_net, const float* scores, const float* lms_net, const int32_t* counts, int rows, int max_out,
                      float* dets, float* lms, int32_t* out_counts, int32_t* flags) {
    std::string why;
    const char* bad = merge_opts_check(o, dets_net, scores, lms_net, counts, rows, max_out, H, W, dets, lms, out_counts, flags);
    if (!bad) bad = frame_geometry_check(FrameGeo{CF_FRAME_BGR, Bf, h, w, 3 * w, 0}, 2, true);
    if (!bad) bad = views_table_check(why, h, w, views, V, H, W);
    if (bad) return fail("cf_op_merge_views", bad);
    MergeParams p{};
    p.kind = MERGE_VIEWS; p.V = V; p.Bf = Bf; p.h = h; p.w = w; p.H = H; p.W = W;
    return op_merge("cf_op_merge_views", device, p, views, (size_t)V * sizeof(cf_view), nullptr, (size_t)Bf * V, "V", o, dets_net, scores,
                    lms_net, counts, rows, max_out, dets, lms, out_counts, flags);
}

int cf_pack_views(const cf_view* views, int V, int Bf, int H, int W, int gutter, cf_place* places, int cap, int* n_places, int* n_canvases) {
    char b[320];
    const char* bad = nullptr;
    if (!views || !n_places || !n_canvases || (cap > 0 && !places)) bad = "null views, places, n_places or n_canvases";
    else if (V < 1) bad = "V must be at least 1";
    else if (Bf < 1) bad = "Bf must be at least 1";
    else if (gutter < 0) bad = "gutter must not be negative";
    else if (cap < 0) bad = "cap must not be negative";
    else if (H < 1 || W < 1) bad = "H and W must be at least 1";
    else if ((long long)V * Bf > INT_MAX) bad = "more than 2^31 placements";
    for (int v = 0; !bad && v < V; ++v) {
        if (views[v].dw < 1 || views[v].dh < 1) { snprintf(b, sizeof b, "view %d has an empty content (dw = %d, dh = %d must be at least 1)", v, views[v].dw, views[v].dh); bad = b; }
        else if (views[v].dw > W || views[v].dh > H) { snprintf(b, sizeof b, "view %d has a content of %d x %d, larger than the canvas %d x %d", v, views[v].dw, views[v].dh, W, H); bad = b; }
    }
    if (bad) return fail("cf_pack_views", bad);
    *n_places = V * Bf;
    return pack_views(views, V, Bf, H, W, gutter, places, cap, n_canvases);
}

// nullptr, or what is wrong with the frames and placements of a packed batch on host frames (the text lives in `why`)
// (rot: the turn of the _rot forms, 0 otherwise: pack_check)
static const char* packed_check(std::string& why, int rot, int format, int Bf, int h, int w, int pitch0, int pitch1, const cf_place* places, int P, int N, int H,
                                int W) {
    if (Bf < 1) return "Bf must be at least 1";
    if (H < 1 || W < 4 || (W & 3)) return "W must be a multiple of 4 and H at least 1";
    if (const char* geo = frame_geometry_check(FrameGeo{format, Bf, h, w, pitch0, pitch1}, 2, true)) return geo;
    return pack_rot_check(why, rot, h, w, places, P, N, Bf, H, W);
}

// The cutter of cf_forward_packed on host frames.
static int op_packed(const char* who, int device, int rot, int format, const cf_yuv_planes* host_frames, int Bf, int h, int w, int pitch0, int pitch1,
                     const cf_place* places, int P, int N, const uint8_t* fill, int H, int W, uint8_t* canvases) {
    std::string why;
    const char* bad = packed_check(why, rot, format, Bf, h, w, pitch0, pitch1, places, P, N, H, W);
    if (!bad) bad = redact_check_planes(format, reinterpret_cast<const void* const*>(host_frames), Bf, 0, pitch0, pitch1);
    if (!bad && (!fill || !canvases)) bad = "null fill or output";
    if (!bad && N > 65535) bad = "more than 65535 canvases";
    if (!bad && (long long)N * H * W * 3 > INT_MAX) bad = "more than 2^31 output bytes";
    if (bad) return fail(who, bad);
    Scope sc(device);
    const std::vector<const void*> dev = up_planes(sc, format, reinterpret_cast<const void* const*>(host_frames), Bf, h, pitch0, pitch1);
    const PackHost t = pack_table(places, P, N, Bf, dev.data(), format);
    const unsigned char* blob = sc.in(t.blob.data(), t.blob.size());
    uint8_t* out = sc.out(canvases, (size_t)N * H * W * 3);
    sc.run([&] { return launch_cut_packed(sc.s, rot, format, pack_dev(t, blob), N, h, w, pitch0, pitch1, fill, out, H, W); });
    return sc.result(who);
}
int cf_op_packed(int device, int format, const cf_yuv_planes* host_frames, int Bf, int h, int w, int pitch0, int pitch1, const cf_place* places,
                 int P, int N, const uint8_t* fill, int H, int W, uint8_t* canvases) {
    return op_packed("cf_op_packed", device, 0, format, host_frames, Bf, h, w, pitch0, pitch1, places, P, N, fill, H, W, canvases);
}
// The cutter of cf_forward_packed_rot on host frames.
int cf_op_packed_rot(int device, int rot, int format, const cf_yuv_planes* host_frames, int Bf, int h, int w, int pitch0, int pitch1,
                     const cf_place* places, int P, int N, const uint8_t* fill, int H, int W, uint8_t* canvases) {
    return op_packed("cf_op_packed_rot", device, rot, format, host_frames, Bf, h, w, pitch0, pitch1, places, P, N, fill, H, W, canvases);
}

static int op_merge_packed(const char* who, int device, int rot, const cf_merge_opts* o, const cf_place* places, int P, int N, int Bf, int h, int w, int H,
                           int W, const float* dets_net, const float* scores, const float* lms_net, const int32_t* counts, int rows, int max_out,
                           float* dets, float* lms, int32_t* out_counts, int32_t* flags) {
    std::string why;
    const char* bad = merge_opts_check(o, dets_net, scores, lms_net, counts, rows, max_out, H, W, dets, lms, out_counts, flags);
    if (!bad) bad = frame_geometry_check(FrameGeo{CF_FRAME_BGR, Bf, h, w, 3 * w, 0}, 2, true);
    if (!bad) bad = pack_rot_check(why, rot, h, w, places, P, N, Bf, H, W);      // (rot 0: pack_check)
    if (bad) return fail(who, bad);
    const PackHost t = pack_table(places, P, N, Bf, nullptr, CF_FRAME_BGR);
    MergeParams p{};
    p.kind = MERGE_PLACED; p.V = t.most; p.Bf = Bf; p.h = h; p.w = w; p.H = H; p.W = W; p.rot = rot;
    return op_merge(who, device, p, t.blob.data(), t.blob.size(), &t, (size_t)N,
                    "most placements of a frame", o, dets_net, scores, lms_net, counts, rows, max_out, dets, lms, out_counts, flags);
}
int cf_op_merge_packed(int device, const cf_merge_opts* o, const cf_place* places, int P, int N, int Bf, int h, int w, int H, int W,
                       const float* dets_net, const float* scores, const float* lms_net, const int32_t* counts, int rows, int max_out,
                       float* dets, float* lms, int32_t* out_counts, int32_t* flags) {
    return op_merge_packed("cf_op_merge_packed", device, 0, o, places, P, N, Bf, h, w, H, W, dets_net, scores, lms_net, counts, rows, max_out, dets, lms,
                           out_counts, flags);
}
// The merge behind cf_forward_packed_rot on host tables: h x w is the STORED frame, the rows come back in its pixels.
int cf_op_merge_packed_rot(int device, int rot, const cf_merge_opts* o, const cf_place* places, int P, int N, int Bf, int h, int w, int H, int W,
                           const float* dets_net, const float* scores, const float* lms_net, const int32_t* counts, int rows, int max_out,
                           float* dets, float* lms, int32_t* out_counts, int32_t* flags) {
    return op_merge_packed("cf_op_merge_packed_rot", device, rot, o, places, P, N, Bf, h, w, H, W, dets_net, scores, lms_net, counts, rows, max_out, dets,
                           lms, out_counts, flags);
}

// nullptr, or what is wrong with the options and sizes of a fit geometry (the text lives in `why`)
static const char* fit_geometry_check(std::string& why, const cf_fit_opts* o, int h, int w, int H, int W) {
    if (const char* bad = fit_check(why, o, CF_FRAME_BGR, 1, h, w, 3 * w, 0, 4, 4)) return bad;      // the options and the frame's sides
    if (H < 1 || W < 1) { why = "H=" + std::to_string(H) + ", W=" + std::to_string(W) + " must be at least 1"; return why.c_str(); }
    return nullptr;
}

int cf_fit_geometry(const cf_fit_opts* o, int h, int w, int H, int W, cf_fit_geom* g) {
    std::string why;
    const char* bad = fit_geometry_check(why, o, h, w, H, W);
    if (!bad && !g) bad = "null output";
    if (bad) return fail("cf_fit_geometry", bad);
    return fit_geometry(o->anchor, o->upscale, h, w, H, W, g);
}

// The fit kernel of cf_forward_fit on host frames.
int cf_op_fit(int device, const cf_fit_opts* o, int format, const cf_yuv_planes* host_frames, int B, int h, int w, int pitch0, int pitch1,
              int H, int W, uint8_t* canvas) {
    const void* const* hp = reinterpret_cast<const void* const*>(host_frames);
    std::string why;
    const char* bad = fit_check(why, o, format, B, h, w, pitch0, pitch1, H, W);
    if (!bad) bad = redact_check_planes(format, hp, B, 0, pitch0, pitch1);
    if (!bad && !canvas) bad = "null output";
    if (!bad && (long long)B * H * W * 3 > INT_MAX) bad = "more than 2^31 output bytes";
    cf_fit_geom g{};
    if (!bad && fit_geometry(o->anchor, o->upscale, h, w, H, W, &g)) bad = "no geometry";
    if (bad) return fail("cf_op_fit", bad);
    Scope sc(device);
    const std::vector<const void*> dev = up_planes(sc, format, hp, B, h, pitch0, pitch1);
    uint8_t* out = sc.out(canvas, (size_t)B * H * W * 3);
    sc.run([&] { return launch_fit_frames(sc.s, 0, format, dev.data(), B, h, w, pitch0, pitch1, g, o->fill, out, H, W); });
    return sc.result("cf_op_fit");
}

int cf_op_unfit(int device, const cf_fit_opts* o, int B, int h, int w, int H, int W, const float* dets_net, const float* scores,
                const float* lms_net, const int32_t* counts, int rows, int max_out, float* dets, float* lms, int32_t* out_counts, int32_t* flags) {
    std::string why;
    const char* bad = fit_geometry_check(why, o, h, w, H, W);
    if (!bad && (!dets_net || !scores || !lms_net || !counts || !dets || !lms || !out_counts || !flags)) bad = "null argument";
    if (!bad && (B < 1 || rows < 1 || max_out < 1)) bad = "B, rows and max_out must be at least 1";
    if (!bad && (long long)B * std::max(rows, max_out) > (1 << 24)) bad = "more than 2^24 rows";
    cf_fit_geom g{};
    if (!bad && fit_geometry(o->anchor, o->upscale, h, w, H, W, &g)) bad = "no geometry";
    if (bad) return fail("cf_op_unfit", bad);
    Scope sc(device);
    const size_t n = (size_t)B * rows, mo = (size_t)B * max_out;
    UnfitParams p{};
    p.g = g; p.h = h; p.w = w; p.B = B;
    p.dets_net = sc.in(dets_net, n * 4);
    p.scores = sc.in(scores, n); p.score_stride = 1;
    p.lms_net = sc.in(lms_net, n * 10);
    p.counts = sc.in(counts, B); p.rows = rows;
    p.max_out = max_out;
    p.dets = sc.inout(dets, mo * 5); p.lms = sc.inout(lms, mo * 10);
    p.corners = sc.make<float>(mo * 4);
    p.out_counts = sc.out(out_counts, B); p.flags = sc.out(flags, B);
    sc.run([&] { return launch_unfit_rows(sc.s, p); });
    return sc.result("cf_op_unfit");
}

// nullptr, or what is wrong with the turn, the options and the sizes of a rotated geometry (the text lives in `why`)
static const char* rot_geometry_check(std::string& why, const cf_rot_opts* o, int h, int w, int H, int W) {
    if (const char* bad = rot_check(why, o, CF_FRAME_BGR, 1, h, w, 3 * w, 0, 4, 4)) return bad;
    if (H < 1 || W < 1) { why = "H=" + std::to_string(H) + ", W=" + std::to_string(W) + " must be at least 1"; return why.c_str(); }
    return nullptr;
}

int cf_rot_geometry(const cf_rot_opts* o, int h, int w, int H, int W, cf_fit_geom* g) {
    std::string why;
    const char* bad = rot_geometry_check(why, o, h, w, H, W);
    if (!bad && !g) bad = "null output";
    if (bad) return fail("cf_rot_geometry", bad);
    return rot_geometry(o, h, w, H, W, g);
}

// The kernel of cf_forward_rot on host frames.
int cf_op_rot(int device, const cf_rot_opts* o, int format, const cf_yuv_planes* host_frames, int B, int h, int w, int pitch0, int pitch1,
              int H, int W, uint8_t* canvas) {
    const void* const* hp = reinterpret_cast<const void* const*>(host_frames);
    std::string why;
    const char* bad = rot_check(why, o, format, B, h, w, pitch0, pitch1, H, W);
    if (!bad) bad = redact_check_planes(format, hp, B, 0, pitch0, pitch1);
    if (!bad && !canvas) bad = "null output";
    if (!bad && (long long)B * H * W * 3 > INT_MAX) bad = "more than 2^31 output bytes";
    cf_fit_geom g{};
    if (!bad && rot_geometry(o, h, w, H, W, &g)) bad = "no geometry";
    if (bad) return fail("cf_op_rot", bad);
    Scope sc(device);
    const std::vector<const void*> dev = up_planes(sc, format, hp, B, h, pitch0, pitch1);
    uint8_t* out = sc.out(canvas, (size_t)B * H * W * 3);
    sc.run([&] { return launch_fit_frames(sc.s, o->rot, format, dev.data(), B, h, w, pitch0, pitch1, g, o->fit.fill, out, H, W); });
    return sc.result("cf_op_rot");
}

int cf_op_unrot(int device, const cf_rot_opts* o, int B, int h, int w, int H, int W, const float* dets_net, const float* scores,
                const float* lms_net, const int32_t* counts, int rows, int max_out, float* dets, float* lms, int32_t* out_counts, int32_t* flags) {
    std::string why;
    const char* bad = rot_geometry_check(why, o, h, w, H, W);
    if (!bad && (!dets_net || !scores || !lms_net || !counts || !dets || !lms || !out_counts || !flags)) bad = "null argument";
    if (!bad && (B < 1 || rows < 1 || max_out < 1)) bad = "B, rows and max_out must be at least 1";
    if (!bad && (long long)B * std::max(rows, max_out) > (1 << 24)) bad = "more than 2^24 rows";
    cf_fit_geom g{};
    if (!bad && rot_geometry(o, h, w, H, W, &g)) bad = "no geometry";
    if (bad) return fail("cf_op_unrot", bad);
    Scope sc(device);
    const size_t n = (size_t)B * rows, mo = (size_t)B * max_out;
    UnfitParams p{};
    p.g = g; p.h = h; p.w = w; p.B = B;
    p.dets_net = sc.in(dets_net, n * 4);
    p.scores = sc.in(scores, n); p.score_stride = 1;
    p.lms_net = sc.in(lms_net, n * 10);
    p.counts = sc.in(counts, B); p.rows = rows;
    p.max_out = max_out;
    p.dets = sc.inout(dets, mo * 5); p.lms = sc.inout(lms, mo * 10);
    p.corners = sc.make<float>(mo * 4);
    p.out_counts = sc.out(out_counts, B); p.flags = sc.out(flags, B);
    sc.run([&] { return launch_unrot_rows(sc.s, p, o->rot); });
    return sc.result("cf_op_unrot");
}

// The mirror kernel of the flip test as the flip forward of a caller's tensor runs it: src -> a 2B batch, whose second half comes back.
int cf_op_mirror(int device, int in_format, const void* x, int B, int H, int W, void* out) {
    std::string why;
    const char* bad = mirror_check(why, in_format, B, H, W);
    if (!bad && (!x || !out)) bad = "null argument";
    const long long one = bad ? 0 : (long long)B * 3 * H * W * (in_format == CF_IN_U8_HWC_BGR ? 1 : 4);
    if (!bad && 2 * one > INT_MAX) bad = "2^31 bytes and more in the doubled batch";
    if (bad) return fail("cf_op_mirror", bad);
    Scope sc(device);
    const void* src = sc.up(x, (size_t)one);
    uint8_t* dst = sc.make<uint8_t>(2 * (size_t)one);
    sc.back(out, dst + one, (size_t)one);
    sc.run([&] { return launch_mirror_batch(sc.s, in_format, src, dst, B, H, W); });
    return sc.result("cf_op_mirror");
}

int cf_op_flip_heads(int device, const float* records_2B, int B, int h, int w, float* records_out, float* hm_plane_out) {
    const char* bad = nullptr;
    if (!records_2B || !records_out || !hm_plane_out) bad = "null argument";
    else if (B < 1 || h < 1 || w < 1) bad = "B, h and w must be at least 1";
    else if (2LL * B * h * w * 16 * (long long)sizeof(float) > INT_MAX) bad = "2^31 bytes and more of records";
    if (bad) return fail("cf_op_flip_heads", bad);
    Scope sc(device);
    const size_t cells = (size_t)B * h * w;
    float* rec = sc.in(records_2B, 2 * cells * 16);
    sc.back(records_out, rec, cells * 16 * sizeof(float));      // the merge happens in place, in the first half
    float* plane = sc.out(hm_plane_out, cells);
    sc.run([&] { return launch_flip_heads(sc.s, rec, plane, B, h, w); });
    return sc.result("cf_op_flip_heads");
}

}  // extern "C"

namespace {

// What cf_op_follow adds to cf_op_track's sequence: the follow of cf_track_follow behind every frame, the update only where `detect` says so
struct OpFollow {
    const cf_follow_opts* o; const uint8_t* detect; int format; const void* const* host_planes; int h, w, pitch0, pitch1, space_h, space_w, tiled;
    int32_t* moves;
};

// The update of cf_track_update, frame after frame, with the state of a fresh tracker (no slot alive, next_id = 1); fw: each frame is then
// followed in its host frames, staged as cf_op_redact stages them.
int op_track_sequence(const char* who, int device, const cf_track_opts* o, int n_streams, int n_frames, int rows, const float* boxes, const float* scores,
                      const float* lms_in, const int32_t* counts_in, float* dets, float* lms, int32_t* info, int32_t* counts, int32_t* flags, const OpFollow* fw,
                      const cf_track_weak_opts* wo = nullptr, const cf_track_motion_opts* mo = nullptr, float* vel = nullptr) {
    const char* bad = track_check(o, n_streams);
    if (!bad) bad = track_weak_check(wo);
    if (!bad) bad = track_motion_check(mo);
    if (!bad && fw) bad = follow_check(fw->o, fw->format, n_streams, fw->h, fw->w, fw->pitch0, fw->pitch1);
    if (!bad && (!boxes || !scores || !lms_in || !counts_in || !dets || !lms || !info || !counts || !flags || (fw && (!fw->detect || !fw->moves)))) bad = "null argument";
    if (!bad && (n_frames < 1 || rows < 1)) bad = "n_frames and rows must be at least 1";
    if (!bad && (long long)n_frames * n_streams * std::max(rows, o->max_tracks) > (1 << 24)) bad = "more than 2^24 rows";
    if (!bad && fw) bad = redact_check_planes(fw->format, fw->host_planes, n_frames * n_streams, 0, fw->pitch0, fw->pitch1);
    if (!bad && fw && (fw->space_h < 1 || fw->space_w < 1 || (fw->tiled != 0 && fw->tiled != 1))) bad = "space_h and space_w must be at least 1, tiled 0 or 1";
    if (!bad && fw && fw->tiled && (fw->space_h != fw->h || fw->space_w != fw->w)) bad = "rows in frame space need space_h x space_w = h x w";
    long long N = 0;
    if (!bad) bad = count_rows(counts_in, n_frames * n_streams, INT_MAX, "negative count", nullptr, &N);
    if (bad) return fail(who, bad);
    Scope sc(device);
    const size_t S = n_streams, F = n_frames, M = o->max_tracks, nin = F * S * rows, nout = F * S * M;
    TrackParams p{};
    p.boxes = sc.in(boxes, nin * 4);
    p.scores = sc.in(scores, nin); p.score_stride = 1;
    p.lms = sc.in(lms_in, nin * 10);
    p.counts = sc.in(counts_in, F * S);
    p.rows = rows; p.B = n_streams; p.stream0 = 0;
    p.iou_thresh = o->iou_thresh; p.max_age = o->max_age; p.min_hits = o->min_hits; p.max_tracks = o->max_tracks; p.hold_grow = o->hold_grow;
    p.set_weak(wo);
    p.set_motion(mo);
    p.meta = sc.make<int>(S * M * 4); p.rec = sc.make<float>(S * M * 16);
    if (mo) { p.vel = sc.make<float>(S * M * 2); p.vel_out = vel ? sc.inout(vel, nout * 2) : nullptr; }
    const std::vector<int> ones(S, 1);
    p.next_id = sc.upv(ones);
    p.dets = sc.inout(dets, nout * 5); p.lms_out = sc.inout(lms, nout * 10); p.info = sc.inout(info, nout * 3);
    p.corners = sc.make<float>(S * M * 4);
    p.out_counts = sc.out(counts, F * S); p.flags = sc.out(flags, F * S);
    FollowParams q{};
    int* moves_dev = nullptr;
    Staged fr;
    if (fw) {
        q.search = fw->o->search; q.max_sad = fw->o->max_sad;
        q.fx = fw->tiled ? 1.0 : (double)fw->w / (double)fw->space_w; q.fy = fw->tiled ? 1.0 : (double)fw->h / (double)fw->space_h;
        q.stream0 = 0; q.max_tracks = o->max_tracks; q.hold_grow = o->hold_grow; q.meta = p.meta; q.rec = p.rec; q.corners = p.corners;
        q.tpl = (uint8_t*)sc.alloc(S * M * kFollowSlotBytes); q.tmeta = (int*)(q.tpl + S * M * kFollowSide * kFollowSide);
        q.slot_moves = sc.make<int>(S * M * 4);
        if (mo) p.tmeta = q.tmeta;
        moves_dev = sc.inout(fw->moves, nout * 4);
        fr = sc.stage(fw->format, fw->host_planes, (int)(F * S), fw->h, fw->w, fw->pitch0, fw->pitch1);      // read only: nothing to copy back
        q.g = fr.geo(n_streams);
    }
    const TrackParams first = p;
    for (size_t f = 0; f < F && sc.ok(); ++f) {
        p.boxes = first.boxes + f * S * rows * 4; p.scores = first.scores + f * S * rows; p.lms = first.lms + f * S * rows * 10;
        p.counts = first.counts + f * S;
        p.dets = first.dets + f * S * M * 5; p.lms_out = first.lms_out + f * S * M * 10; p.info = first.info + f * S * M * 3;
        p.out_counts = first.out_counts + f * S; p.flags = first.flags + f * S;
        if (first.vel_out) p.vel_out = first.vel_out + f * S * M * 2;
        if (!fw || fw->detect[f]) sc.run([&] { return launch_track_update(sc.s, p); });
        if (!fw) continue;
        q.planes = fr.planes(f * S);
        q.dets = p.dets; q.lms_out = p.lms_out; q.info = p.info; q.out_counts = p.out_counts; q.moves = moves_dev + f * S * M * 4;
        sc.run([&] { return launch_track_follow(sc.s, q); });
    }
    return sc.result(who);
}

}  // namespace

extern "C" {

int cf_op_track(int device, const cf_track_opts* o, int n_streams, int n_frames, int rows, const float* boxes, const float* scores,
                const float* lms_in, const int32_t* counts_in, float* dets, float* lms, int32_t* info, int32_t* counts, int32_t* flags) {
    return op_track_sequence("cf_op_track", device, o, n_streams, n_frames, rows, boxes, scores, lms_in, counts_in, dets, lms, info, counts, flags, nullptr);
}

int cf_op_track_weak(int device, const cf_track_opts* o, const cf_track_weak_opts* weak, int n_streams, int n_frames, int rows, const float* boxes,
                     const float* scores, const float* lms_in, const int32_t* counts_in, float* dets, float* lms, int32_t* info, int32_t* counts, int32_t* flags) {
    if (!weak) return cf_op_track(device, o, n_streams, n_frames, rows, boxes, scores, lms_in, counts_in, dets, lms, info, counts, flags);
    return op_track_sequence("cf_op_track_weak", device, o, n_streams, n_frames, rows, boxes, scores, lms_in, counts_in, dets, lms, info, counts, flags, nullptr, weak);
}

int cf_op_follow(int device, const cf_track_opts* o, const cf_follow_opts* fo, int n_streams, int n_frames, int rows, const float* boxes,
                 const float* scores, const float* lms_in, const int32_t* counts_in, const uint8_t* detect, int format,
                 const cf_planes_rw* frames, int h, int w, int pitch0, int pitch1, int space_h, int space_w, int tiled, float* dets,
                 float* lms, int32_t* info, int32_t* counts, int32_t* flags, int32_t* moves) {
    const OpFollow fw{fo, detect, format, reinterpret_cast<const void* const*>(frames), h, w, pitch0, pitch1, space_h, space_w, tiled, moves};
    return op_track_sequence("cf_op_follow", device, o, n_streams, n_frames, rows, boxes, scores, lms_in, counts_in, dets, lms, info, counts, flags, &fw);
}

int cf_op_track_ex(int device, const cf_track_opts* o, const cf_track_weak_opts* weak, const cf_track_motion_opts* motion, int n_streams, int n_frames,
                   int rows, const float* boxes, const float* scores, const float* lms_in, const int32_t* counts_in, float* dets, float* lms, int32_t* info,
                   int32_t* counts, int32_t* flags, float* vel) {
    if (!motion) return cf_op_track_weak(device, o, weak, n_streams, n_frames, rows, boxes, scores, lms_in, counts_in, dets, lms, info, counts, flags);
    return op_track_sequence("cf_op_track_ex", device, o, n_streams, n_frames, rows, boxes, scores, lms_in, counts_in, dets, lms, info, counts, flags, nullptr,
                             weak, motion, vel);
}

int cf_op_follow_ex(int device, const cf_track_opts* o, const cf_track_weak_opts* weak, const cf_track_motion_opts* motion, const cf_follow_opts* fo,
                    int n_streams, int n_frames, int rows, const float* boxes, const float* scores, const float* lms_in, const int32_t* counts_in,
                    const uint8_t* detect, int format, const cf_planes_rw* frames, int h, int w, int pitch0, int pitch1, int space_h, int space_w, int tiled,
                    float* dets, float* lms, int32_t* info, int32_t* counts, int32_t* flags, int32_t* moves) {
    if (!weak && !motion)
        return cf_op_follow(device, o, fo, n_streams, n_frames, rows, boxes, scores, lms_in, counts_in, detect, format, frames, h, w, pitch0, pitch1, space_h,
                            space_w, tiled, dets, lms, info, counts, flags, moves);
    const OpFollow fw{fo, detect, format, reinterpret_cast<const void* const*>(frames), h, w, pitch0, pitch1, space_h, space_w, tiled, moves};
    return op_track_sequence("cf_op_follow_ex", device, o, n_streams, n_frames, rows, boxes, scores, lms_in, counts_in, dets, lms, info, counts, flags, &fw,
                             weak, motion);
}

// The kernels of cf_scene_check over a sequence of host frames, with the state of a fresh cf_scene (nothing valid) and no tracker.
int cf_op_scene(int device, const cf_scene_opts* o, int n_streams, int n_frames, int format, const cf_planes_rw* frames, int h, int w, int pitch0,
                int pitch1, int32_t* out, int32_t* sigs) {
    const void* const* host_planes = reinterpret_cast<const void* const*>(frames);
    const char* bad = !o ? "null options" : nullptr;
    if (!bad && (n_streams < 1 || n_streams > kTrackMaxStreams)) bad = "n_streams must be in 1..4096";
    if (!bad && n_frames < 1) bad = "n_frames must be at least 1";
    if (!bad) bad = scene_check(o, format, n_streams, h, w, pitch0, pitch1);
    if (!bad && (long long)n_frames * n_streams > (1 << 24)) bad = "more than 2^24 frames";
    if (!bad) bad = redact_check_planes(format, host_planes, n_frames * n_streams, 0, pitch0, pitch1);
    if (!bad && !out) bad = "null out";
    if (bad) return fail("cf_op_scene", bad);
    Scope sc(device);
    const size_t S = n_streams, F = n_frames;
    SceneParams p{};
    p.hist_thresh = o->hist_thresh; p.grid_thresh = o->grid_thresh; p.stream0 = 0;
    p.sig = sc.make<int>(S * kSceneSig); p.st = sc.make<int>(S * 4);
    p.part = (int*)sc.alloc(scene_part_bytes(n_streams, h));
    int* out_dev = sc.out(out, F * S * 4);
    int* sig_dev = sigs ? sc.out(sigs, F * S * kSceneSig) : nullptr;
    const Staged fr = sc.stage(format, host_planes, (int)(F * S), h, w, pitch0, pitch1);      // read only: nothing to copy back
    p.g = fr.geo(n_streams);
    for (size_t f = 0; f < F && sc.ok(); ++f) {
        p.planes = fr.planes(f * S); p.out = out_dev + f * S * 4; p.sig_out = sig_dev ? sig_dev + f * S * kSceneSig : nullptr;
        sc.run([&] { return launch_scene_check(sc.s, p); });
    }
    return sc.result("cf_op_scene");
}

}  // extern "C"

namespace {

// What cf_op_lookback_trace adds to cf_op_lookback's sequence: the object is enabled, and every push has its frame
struct OpTrace {
    const cf_follow_opts* o; int format; const void* const* host_planes; int h, w, pitch0, pitch1, space_h, space_w, tiled;
    int32_t* moves;
};

// The kernel of cf_lookback_step over a sequence of host tables, with the state of a fresh cf_lookback (empty queues, max_id = seq_next = 0);
// tr: of an enabled one, the frames staged as cf_op_redact stages them, retain and trace ahead of every push.
int op_lookback_sequence(const char* who, int device, const cf_lookback_opts* o, int n_streams, int n_steps, int rows_in, const uint8_t* push, const float* dets_in,
                         const float* lms_in, const int32_t* info_in, const int32_t* counts_in, const int32_t* cuts, float* dets, float* lms,
                         int32_t* info, int32_t* counts, int32_t* state, const OpTrace* tr) {
    const char* bad = lookback_check(o, n_streams);
    if (!bad && tr) bad = follow_check(tr->o, tr->format, n_streams, tr->h, tr->w, tr->pitch0, tr->pitch1);
    if (!bad && tr && (((tr->h | tr->w) & 1) || tr->h < 2 || tr->w < 2)) bad = "h and w must be even and in [2, 8192]";
    if (!bad && (!push || !dets_in || !lms_in || !info_in || !counts_in || !dets || !lms || !info || !counts || !state || (tr && !tr->moves))) bad = "null argument";
    if (!bad && n_steps < 1) bad = "n_steps must be at least 1";
    if (!bad && (rows_in < 1 || rows_in > o->rows)) bad = "rows_in must be in 1..rows";
    if (!bad && (long long)n_steps * n_streams * o->rows > (1 << 24)) bad = "more than 2^24 rows";
    if (!bad && tr) bad = redact_check_planes(tr->format, tr->host_planes, n_steps * n_streams, 0, tr->pitch0, tr->pitch1);
    if (!bad && tr && (tr->space_h < 1 || tr->space_w < 1 || (tr->tiled != 0 && tr->tiled != 1))) bad = "space_h and space_w must be at least 1, tiled 0 or 1";
    if (!bad && tr && tr->tiled && (tr->space_h != tr->h || tr->space_w != tr->w)) bad = "rows in frame space need space_h x space_w = h x w";
    if (bad) return fail(who, bad);
    Scope sc(device);
    const size_t S = n_streams, F = n_steps, R = o->rows, cap = (size_t)o->depth + 1, nin = F * S * rows_in, nout = F * S * R;
    std::vector<int32_t> codes(F * S * 4, 0), ones(S, 1);
    for (size_t k = 0; k < F * S; ++k) codes[k * 4] = cuts && (cuts[k] & 1) ? CF_SCENE_CUT : CF_SCENE_SAME;
    LookbackParams p{};
    p.depth = o->depth; p.rows = o->rows; p.confirm = o->confirm; p.grow = o->grow; p.stream0 = 0; p.B = n_streams;
    p.in_dets = sc.in(dets_in, nin * 5); p.in_lms = sc.in(lms_in, nin * 10); p.in_info = sc.in(info_in, nin * 3); p.in_counts = sc.in(counts_in, F * S);
    p.scene = sc.upv(codes);
    const int* one = sc.upv(ones);
    p.in_stride = rows_in;
    p.qmeta = sc.make<int>(S * 4); p.pend = sc.make<int>(S); p.emeta = sc.make<int>(S * cap * 4);
    p.rec = sc.make<float>(S * cap * R * 16); p.info = sc.make<int>(S * cap * R * 4);
    p.dets = sc.inout(dets, nout * 5); p.lms = sc.inout(lms, nout * 10); p.out_info = sc.inout(info, nout * 3);
    p.counts = sc.out(counts, F * S); p.state = sc.out(state, F * S * 4);
    LookbackTraceParams q{};
    Staged fr;
    if (tr) {
        q.search = tr->o->search; q.max_sad = tr->o->max_sad;
        q.fx = tr->tiled ? 1.0 : (double)tr->w / (double)tr->space_w; q.fy = tr->tiled ? 1.0 : (double)tr->h / (double)tr->space_h;
        q.luma = (uint8_t*)sc.alloc(S * cap * tr->h * lookback_luma_pitch(tr->w));
        q.trace = sc.make<int>(S * cap * R * o->depth * 4);
        p.trace = q.trace; p.fx = q.fx; p.fy = q.fy; p.moves = sc.inout(tr->moves, nout * 4);
        fr = sc.stage(tr->format, tr->host_planes, (int)(F * S), tr->h, tr->w, tr->pitch0, tr->pitch1);      // read only: nothing to copy back
        q.g = fr.geo(n_streams);
    }
    const LookbackParams first = p;
    for (size_t f = 0; f < F && sc.ok(); ++f) {
        for (size_t s = 0; cuts && s < S; ++s)      // cf_lookback_forget of stream s
            if (cuts[f * S + s] & 2) sc.run([&] { return hipMemcpyAsync(p.pend + s, one + s, sizeof(int), hipMemcpyDeviceToDevice, sc.s); });
        p.push = push[f] ? 1 : 0;
        p.in_dets = first.in_dets + f * S * rows_in * 5; p.in_lms = first.in_lms + f * S * rows_in * 10; p.in_info = first.in_info + f * S * rows_in * 3;
        p.in_counts = first.in_counts + f * S;
        p.scene = cuts ? first.scene + f * S * 4 : nullptr;
        p.dets = first.dets + f * S * R * 5; p.lms = first.lms + f * S * R * 10; p.out_info = first.out_info + f * S * R * 3;
        p.counts = first.counts + f * S; p.state = first.state + f * S * 4;
        if (tr) p.moves = first.moves + f * S * R * 4;
        if (tr && p.push) {
            q.planes = fr.planes(f * S); q.step = p;
            sc.run([&] { return launch_lookback_trace(sc.s, q); });
        }
        sc.run([&] { return launch_lookback_step(sc.s, p); });
    }
    return sc.result(who);
}

}  // namespace

extern "C" {

int cf_op_lookback(int device, const cf_lookback_opts* o, int n_streams, int n_steps, int rows_in, const uint8_t* push, const float* dets_in,
                   const float* lms_in, const int32_t* info_in, const int32_t* counts_in, const int32_t* cuts, float* dets, float* lms,
                   int32_t* info, int32_t* counts, int32_t* state) {
    return op_lookback_sequence("cf_op_lookback", device, o, n_streams, n_steps, rows_in, push, dets_in, lms_in, info_in, counts_in, cuts, dets, lms, info, counts,
                                state, nullptr);
}

int cf_op_lookback_trace(int device, const cf_lookback_opts* o, const cf_follow_opts* fo, int n_streams, int n_steps, int rows_in, const uint8_t* push,
                         const float* dets_in, const float* lms_in, const int32_t* info_in, const int32_t* counts_in, const int32_t* cuts, int format,
                         const cf_planes_rw* frames, int h, int w, int pitch0, int pitch1, int space_h, int space_w, int tiled, float* dets, float* lms,
                         int32_t* info, int32_t* counts, int32_t* state, int32_t* moves) {
    const OpTrace tr{fo, format, reinterpret_cast<const void* const*>(frames), h, w, pitch0, pitch1, space_h, space_w, tiled, moves};
    return op_lookback_sequence("cf_op_lookback_trace", device, o, n_streams, n_steps, rows_in, push, dets_in, lms_in, info_in, counts_in, cuts, dets, lms, info,
                                counts, state, &tr);
}

// The score kernel of cf_bestshot_offer alone: one image whose n rows all count and are eligible (ids 1 .. n, hits 1000, misses 0).
int cf_op_chip_quality(int device, const cf_bestshot_opts* o, const uint8_t* chips, const float* boxes, const float* scores, const float* lms,
                       int n, double fx, double fy, int64_t* quality, int32_t* parts) {
    const char* bad = best_check(o, 1);
    if (!bad && (!chips || !boxes || !scores || !lms || !quality || !parts)) bad = "null argument";
    if (!bad && (n < 1 || n > 65536)) bad = "n must be in 1..65536";
    if (!bad && (!std::isfinite(fx) || !std::isfinite(fy) || !(fx > 0) || !(fy > 0))) bad = "fx and fy must be finite and greater than 0";
    if (bad) return fail("cf_op_chip_quality", bad);
    Scope sc(device);
    std::vector<int32_t> info((size_t)n * 3);
    for (int i = 0; i < n; ++i) { info[(size_t)i * 3] = i + 1; info[(size_t)i * 3 + 1] = 1000; info[(size_t)i * 3 + 2] = 0; }
    const int offs[2] = {0, n};
    BestOffer p{};
    p.t.size = o->size; p.t.entries = o->entries; p.t.min_hits = o->min_hits; p.t.terms = o->terms;
    p.r = BestRows{sc.in(boxes, (size_t)n * 4), sc.in(scores, n), 1, sc.in(lms, (size_t)n * 10), sc.upv(info), sc.in(&offs[1], 1), n};
    p.B = 1; p.cap_faces = n; p.fx = fx; p.fy = fy;
    p.chips = sc.in(chips, (size_t)n * best_chip_bytes(o->size));
    p.offsets = sc.in(offs, 2);
    p.q = (long long*)sc.out(quality, n); p.sc = sc.make<int32_t>((size_t)n * kBestScratchInts);
    sc.run([&] { return hipStreamSynchronize(sc.s); });       // (offs and info are on this stack frame)
    sc.run([&] { return launch_best_score(sc.s, p); });
    // the first four of a row's scratch ints (a strided read, not a declared output)
    sc.run([&] { return hipMemcpy2DAsync(parts, 4 * sizeof(int32_t), p.sc, kBestScratchInts * sizeof(int32_t), 4 * sizeof(int32_t), n, hipMemcpyDeviceToHost, sc.s); });
    return sc.result("cf_op_chip_quality");
}

// cf_bestshot_offer and cf_bestshot_collect, frame after frame, with the state of a fresh table (every entry FREE, t = seq = 0)
int cf_op_bestshot(int device, const cf_bestshot_opts* o, int n_streams, int n_frames, int rows, const float* boxes, const float* scores,
                   const float* lms, const int32_t* info, const int32_t* counts, const int32_t* chip_counts, const uint8_t* chips,
                   const uint8_t* collect, int cap, double fx, double fy, uint8_t* out_chips, int64_t* out_quality, int32_t* out_records,
                   float* out_dets, float* out_lms, int32_t* out_counts, int32_t* out_pending, int32_t* out_flags, int32_t* offer_flags,
                   int64_t* offer_quality) {
    const char* bad = best_check(o, n_streams);
    if (!bad && (!boxes || !scores || !lms || !info || !counts || !chip_counts || !chips || !collect || !out_chips || !out_quality || !out_records ||
                 !out_dets || !out_lms || !out_counts || !out_pending || !out_flags || !offer_flags || !offer_quality)) bad = "null argument";
    if (!bad && n_frames < 1) bad = "n_frames must be at least 1";
    if (!bad && (rows < 1 || rows > kBestMaxRows)) bad = "rows must be in 1..1024";
    if (!bad && (cap < 0 || cap > o->entries)) bad = "cap must be in 0..entries";
    if (!bad && (!std::isfinite(fx) || !std::isfinite(fy) || !(fx > 0) || !(fy > 0))) bad = "fx and fy must be finite and greater than 0";
    if (!bad && (long long)n_frames * n_streams * std::max(rows, std::max(cap, 1)) > (1 << 24)) bad = "more than 2^24 rows";
    const size_t S = bad ? 0 : n_streams, F = bad ? 0 : n_frames, one = bad ? 0 : best_chip_bytes(o->size), E = bad ? 0 : o->entries;
    if (!bad) for (size_t k = 0; k < F * S; ++k) if (counts[k] < 0 || chip_counts[k] < 0) { bad = "negative count"; break; }
    if (!bad) for (size_t f = 0; f < F; ++f) if (collect[f] > 2) { bad = "collect must be 0, 1 or 2"; break; }
    // the chips of every frame, packed as an align call packs them: offsets [F][S + 1] within the frame, base[f] chips before frame f
    std::vector<int> offs(F * (S + 1)), base(F + 1, 0);
    if (!bad) {
        for (size_t f = 0; f < F; ++f) {
            int off = 0;
            for (size_t s = 0; s < S; ++s) { offs[f * (S + 1) + s] = off; off += std::min(chip_counts[f * S + s], rows); }
            offs[f * (S + 1) + S] = off; base[f + 1] = base[f] + off;
        }
        if ((double)base[F] * (double)one > 1073741824.0 || (double)S * E * (double)one > 1073741824.0 || (double)F * S * std::max(cap, 1) * (double)one > 1073741824.0)
            bad = "more than 1 GiB of chips";
    }
    if (bad) return fail("cf_op_bestshot", bad);
    Scope sc(device);
    std::vector<uint8_t> packed(std::max<size_t>((size_t)base[F] * one, 16));
    for (size_t f = 0; f < F; ++f)
        for (size_t s = 0; s < S; ++s) {
            const size_t m = (size_t)(offs[f * (S + 1) + s + 1] - offs[f * (S + 1) + s]);
            if (m) memcpy(packed.data() + ((size_t)base[f] + offs[f * (S + 1) + s]) * one, chips + (f * S + s) * rows * one, m * one);
        }
    const size_t nin = F * S * rows, nout = F * S * cap, nq = std::max<size_t>(base[F], 1);
    std::vector<long long> q(nq);
    BestOffer p{};
    p.t = BestTable{o->size, o->entries, o->min_hits, o->terms, sc.make<int32_t>(S * E * kBestRecInts), sc.make<float>(S * E * kBestRowFloats),
                    sc.make<uint8_t>(S * E * one), sc.make<int32_t>(S * kBestStreamInts)};
    p.r = BestRows{sc.in(boxes, nin * 4), sc.in(scores, nin), 1, sc.in(lms, nin * 10), sc.in(info, nin * 3), sc.in(counts, F * S), rows};
    p.stream0 = 0; p.B = n_streams; p.fx = fx; p.fy = fy;
    p.chips = sc.upv(packed); p.offsets = sc.upv(offs);
    p.q = sc.make<long long>(nq); p.sc = sc.make<int32_t>(nq * kBestScratchInts);
    sc.back(q.data(), p.q, (size_t)base[F] * sizeof(long long));      // the chips' qualities: scattered to offer_quality's rows below
    p.jobs = sc.make<int32_t>(S * rows * 2); p.flags = sc.out(offer_flags, F * S);
    BestCollect c{};
    c.t = p.t; c.stream0 = 0; c.B = n_streams; c.cap = cap;
    c.chips = sc.inout(out_chips, nout * one); c.quality = (long long*)sc.inout(out_quality, nout);
    c.records = sc.inout(out_records, nout * 8); c.dets = sc.inout(out_dets, nout * 5); c.lms = sc.inout(out_lms, nout * 10);
    c.counts = sc.out(out_counts, F * S); c.pending = sc.out(out_pending, F * S); c.flags = sc.out(out_flags, F * S);
    c.jobs = sc.make<int32_t>(S * std::max(cap, 1) * 2);
    const BestOffer p0 = p;
    const BestCollect c0 = c;
    for (size_t f = 0; f < F && sc.ok(); ++f) {
        p.r.boxes = p0.r.boxes + f * S * rows * 4; p.r.scores = p0.r.scores + f * S * rows; p.r.lms = p0.r.lms + f * S * rows * 10;
        p.r.info = p0.r.info + f * S * rows * 3; p.r.counts = p0.r.counts + f * S;
        p.chips = p0.chips + (size_t)base[f] * one; p.offsets = p0.offsets + f * (S + 1); p.cap_faces = base[f + 1] - base[f];
        p.q = p0.q + base[f]; p.sc = p0.sc + (size_t)base[f] * kBestScratchInts; p.flags = p0.flags + f * S;
        sc.run([&] { return launch_best_offer(sc.s, p); });
        if (!collect[f]) continue;
        c.flush = collect[f] == 2;
        c.chips = (uint8_t*)c0.chips + f * S * cap * one; c.quality = c0.quality + f * S * cap; c.records = c0.records + f * S * cap * 8;
        c.dets = c0.dets + f * S * cap * 5; c.lms = c0.lms + f * S * cap * 10;
        c.counts = c0.counts + f * S; c.pending = c0.pending + f * S; c.flags = c0.flags + f * S;
        sc.run([&] { return launch_best_collect(sc.s, c); });
    }
    const int r = sc.result("cf_op_bestshot");
    if (r != CF_OK) return r;
    for (size_t k = 0; k < nin; ++k) offer_quality[k] = -1;
    for (size_t f = 0; f < F; ++f)
        for (size_t s = 0; s < S; ++s) {
            const int o0 = offs[f * (S + 1) + s], m = offs[f * (S + 1) + s + 1] - o0;
            for (int i = 0; i < m; ++i) offer_quality[(f * S + s) * rows + i] = q[(size_t)base[f] + o0 + i];
        }
    return CF_OK;
}

}  // extern "C"
