// The arithmetic of cf_draw_faces as the host (cf_draw_layout) and the kernels (cf_draw.hip) share it: the point mapping of step 1 of the
// statement in include/centerface_hip.h, the integer geometry of one row (DrawFace), the layer a row puts on a frame pixel (draw_layer)
// and the glyph table.  tests/draw_cases.py restates it in numpy; both sides are equal field for field and byte for byte.  Every file
// that includes this one is compiled with -ffp-contract=off or is host code: the mapping rounds every operation.
//
//   P(v, f) = (int)min(max(floor(v * f), -8192.0), 16384.0)
//   outline: inside [X1..X2] x [Y1..Y2] with x < X1 + t || x > X2 - t || y < Y1 + t || y > Y2 - t; a held row with dash_held keeps
//            the pixels with ((x + y) % (8 * t)) < 4 * t
//   dot:     dx*dx + dy*dy <= r*r + r about (Lx, Ly), live rows only
//   plate:   [x0, x0 + Pw) x [y0, y0 + Ph), Pw = k * (6n + 1), Ph = 9k; ink: u = (x - x0) / k, v = (y - y0) / k, 1 <= v <= 7, u >= 1,
//            q = (u - 1) / 6 < n, col = (u - 1) % 6 < 5, bit 4 - col of GLYPH[digit q][v - 1]
//   layers:  1 held outline / plate, 2 live outline / plate, 3 ink, 4 dot; a pixel takes the highest
#pragma once
#include <math.h>
#include <stdint.h>

#include <hip/hip_runtime.h>

#include "centerface_hip.h"

namespace cf {

// GLYPH, rows top to bottom, 5 bits each, MSB = left column:
//   0: 0E 11 13 15 19 11 0E    1: 04 0C 04 04 04 04 0E    2: 0E 11 01 02 04 08 1F    3: 1F 02 04 02 01 11 0E
//   4: 02 06 0A 12 1F 02 02    5: 1F 10 1E 01 01 11 0E    6: 06 08 10 1E 11 11 0E    7: 1F 01 02 04 08 08 08
//   8: 0E 11 11 0E 11 11 0E    9: 0E 11 11 0F 01 02 0C
// as one 35-bit word per digit (row v - 1 in bits 5 * (v - 1) .. 5 * (v - 1) + 4): a table of constants the compiler folds into the code
__host__ __device__ inline unsigned draw_glyph_row(int digit, int row) {
    constexpr unsigned long long G[10] = {
#define CF_GLYPH(a, b, c, d, e, f, g) ((unsigned long long)0x##a | (unsigned long long)0x##b << 5 | (unsigned long long)0x##c << 10 | (unsigned long long)0x##d << 15 | \
                                       (unsigned long long)0x##e << 20 | (unsigned long long)0x##f << 25 | (unsigned long long)0x##g << 30)
        CF_GLYPH(0E, 11, 13, 15, 19, 11, 0E), CF_GLYPH(04, 0C, 04, 04, 04, 04, 0E), CF_GLYPH(0E, 11, 01, 02, 04, 08, 1F), CF_GLYPH(1F, 02, 04, 02, 01, 11, 0E),
        CF_GLYPH(02, 06, 0A, 12, 1F, 02, 02), CF_GLYPH(1F, 10, 1E, 01, 01, 11, 0E), CF_GLYPH(06, 08, 10, 1E, 11, 11, 0E), CF_GLYPH(1F, 01, 02, 04, 08, 08, 08),
        CF_GLYPH(0E, 11, 11, 0E, 11, 11, 0E), CF_GLYPH(0E, 11, 11, 0F, 01, 02, 0C)
#undef CF_GLYPH
    };
    return (unsigned)(G[digit] >> (5 * row)) & 31u;
}

// the options of one call, as cf_draw_opts without the colours
struct DrawGeoOpts { int what, t, r, label, k, dash; float scale; };

// One row's integer geometry: the 32 int32 of cf_draw_layout, in its order.  ok = 0 (a skipped row): every other field is 0.
struct DrawFace {
    int32_t ok;
    int32_t X1, Y1, X2, Y2;      // the box, both corners inclusive
    int32_t held;                // misses > 0
    int32_t px0, py0, pw, ph;    // the plate [px0, px0 + pw) x [py0, py0 + ph); all 0 without a label
    int32_t n;                   // digits of the label, 0 = none
    int32_t digit[10];           // digit[q], q < n, most significant first; 0 past n
    int32_t lvalid;              // bit j: landmark j is finite
    int32_t lxy[10];             // Lx0, Ly0, .. Lx4, Ly4; 0 where not valid
};
static_assert(sizeof(DrawFace) == 32 * sizeof(int32_t), "DrawFace is the out[32] of cf_draw_layout");

__host__ __device__ inline int draw_point(double v, double f) { return (int)fmin(fmax(floor(v * f), -8192.0), 16384.0); }

// box [4], score, lms [10] or nullptr, info [3] = id, hits, misses or nullptr -> the record of the row in an h x w frame, rows in H x W
__host__ __device__ inline DrawFace draw_face(const DrawGeoOpts& o, const float* bx, float score, const float* lms, const int32_t* info,
                                              int h, int w, int H, int W) {
    DrawFace f{};
    const double x1 = (double)bx[0], y1 = (double)bx[1], x2 = (double)bx[2], y2 = (double)bx[3], s = (double)o.scale;
    const double cx = (x1 + x2) * 0.5, cy = (y1 + y2) * 0.5;
    const double hw = (x2 - x1) * 0.5 * s, hh = (y2 - y1) * 0.5 * s;
    const double fx = (double)w / (double)W, fy = (double)h / (double)H;
    if (!(isfinite(x1) && isfinite(y1) && isfinite(x2) && isfinite(y2) && hw > 0.0 && hh > 0.0)) return f;
    f.ok = 1;
    f.X1 = draw_point(cx - hw, fx); f.X2 = draw_point(cx + hw, fx);
    f.Y1 = draw_point(cy - hh, fy); f.Y2 = draw_point(cy + hh, fy);
    f.held = info && info[2] > 0 ? 1 : 0;
    for (int j = 0; lms && j < 5; ++j) {
        const double lx = (double)lms[2 * j], ly = (double)lms[2 * j + 1];
        if (!(isfinite(lx) && isfinite(ly))) continue;
        f.lvalid |= 1 << j;
        f.lxy[2 * j] = draw_point(lx, fx); f.lxy[2 * j + 1] = draw_point(ly, fy);
    }
    long long value = -1;
    if (o.label == CF_DRAW_LABEL_SCORE && isfinite((double)score)) value = (long long)fmin(fmax(floor((double)score * 100.0), 0.0), 100.0);
    if (o.label == CF_DRAW_LABEL_ID && info && info[0] > 0) value = info[0];
    if (value >= 0) {
        int n = 1;
        for (long long v = value; v >= 10; v /= 10) ++n;
        f.n = n;
        for (int q = n - 1; q >= 0; --q) { f.digit[q] = (int32_t)(value % 10); value /= 10; }
        f.pw = o.k * (6 * n + 1); f.ph = 9 * o.k;
        f.px0 = f.X1; f.py0 = f.Y1 - f.ph >= 0 ? f.Y1 - f.ph : f.Y1 + o.t;
    }
    return f;
}

// the layer (0 = none) that the row puts on the frame pixel (x, y), x, y >= 0
__host__ __device__ inline int draw_layer(const DrawFace& f, const DrawGeoOpts& o, int x, int y) {
    if (!f.ok) return 0;
    if ((o.what & CF_DRAW_LANDMARKS) && !f.held) {
        const int rr = o.r * o.r + o.r;
        for (int j = 0; j < 5; ++j) {
            if (!(f.lvalid >> j & 1)) continue;
            const int dx = x - f.lxy[2 * j], dy = y - f.lxy[2 * j + 1];
            if (dx*dx + dy*dy <= rr) return 4;
        }
    }
    const int base = f.held ? 1 : 2;
    int layer = 0;
    if (f.n > 0 && x >= f.px0 && x < f.px0 + f.pw && y >= f.py0 && y < f.py0 + f.ph) {
        const int u = (x - f.px0) / o.k, v = (y - f.py0) / o.k;
        if (v >= 1 && v <= 7 && u >= 1) {
            const int q = (u - 1) / 6, col = (u - 1) % 6;
            if (q < f.n && col < 5 && (draw_glyph_row(f.digit[q], v - 1) >> (4 - col) & 1u)) return 3;
        }
        layer = base;
    }
    if ((o.what & CF_DRAW_BOX) && x >= f.X1 && x <= f.X2 && y >= f.Y1 && y <= f.Y2 &&
        (x < f.X1 + o.t || x > f.X2 - o.t || y < f.Y1 + o.t || y > f.Y2 - o.t) &&
        !(f.held && o.dash && ((x + y) % (8 * o.t)) >= 4 * o.t))
        layer = base;
    return layer;
}

// the rectangle [x0, x1) x [y0, y1) of the frame that holds every primitive of the row (empty: x0 >= x1 or y0 >= y1)
struct DrawRect { int32_t x0, y0, x1, y1; };
__host__ __device__ inline DrawRect draw_bounds(const DrawFace& f, const DrawGeoOpts& o, int h, int w) {
    DrawRect b{w, h, 0, 0};
    if (!f.ok) return b;
    auto add = [&](int xa, int ya, int xb, int yb) {      // inclusive corners
        b.x0 = xa < b.x0 ? xa : b.x0; b.y0 = ya < b.y0 ? ya : b.y0; b.x1 = xb + 1 > b.x1 ? xb + 1 : b.x1; b.y1 = yb + 1 > b.y1 ? yb + 1 : b.y1;
    };
    if (o.what & CF_DRAW_BOX) add(f.X1, f.Y1, f.X2, f.Y2);
    if (f.n > 0) add(f.px0, f.py0, f.px0 + f.pw - 1, f.py0 + f.ph - 1);
    if ((o.what & CF_DRAW_LANDMARKS) && !f.held)
        for (int j = 0; j < 5; ++j)
            if (f.lvalid >> j & 1) add(f.lxy[2 * j] - o.r, f.lxy[2 * j + 1] - o.r, f.lxy[2 * j] + o.r, f.lxy[2 * j + 1] + o.r);
    b.x0 = b.x0 < 0 ? 0 : b.x0; b.y0 = b.y0 < 0 ? 0 : b.y0; b.x1 = b.x1 > w ? w : b.x1; b.y1 = b.y1 > h ? h : b.y1;
    return b;
}

// what draw_prep_kernel leaves per (image, row) for draw_paint_kernel
struct DrawRec { DrawFace f; DrawRect b; };

}  // namespace cf
