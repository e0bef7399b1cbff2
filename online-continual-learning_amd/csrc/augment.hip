// K13: SCR's view augmentation (random resized crop, flip, colour jitter in one of 24 orders, grayscale) as two kernels: the per-image
// parameters from raw uniform draws, then one thread per output pixel.
#include "small_ops.h"
#include <math.h>

using namespace ocl;

// =====================================================================================================
// K13 SCR view augmentation (parameters drawn on the host)
// =====================================================================================================
namespace ocl {
// augment_kernel: one thread per output pixel, one grid row per image.  grid.y cannot exceed 65535, and the kernel forms the pixel
// index (up to the last workgroup's end) and h * w in int: larger sizes are refused here, before a launch.  n = 0: no launch.
SPlan plan_augment(int64_t n, int64_t h, int64_t w) {
    if (n > 65535 || h * w > (int64_t)0x7fffffff - 255) return splan(OCL_PATH_AUGMENT_REFUSED);
    if (n == 0) return splan(OCL_PATH_AUGMENT);
    return splan(OCL_PATH_AUGMENT, (unsigned)((h * w + 255) / 256), (unsigned)n, 256);
}
SPlan plan_aug_params(int64_t n) { return splan(OCL_PATH_AUG_PARAMS, (unsigned)((n + 63) / 64), 1, 64); }
}  // namespace ocl

__device__ __forceinline__ float clamp01(float v) { return fminf(fmaxf(v, 0.f), 1.f); }

__device__ __forceinline__ void rgb2hsv(float r, float g, float b, float& h, float& s, float& v) {
    const float mx = fmaxf(r, fmaxf(g, b)), mn = fminf(r, fminf(g, b));
    const float df = mx - mn;
    v = mx;
    s = mx > 0.f ? df / mx : 0.f;
    if (df <= 0.f) {
        h = 0.f;
    } else if (mx == r) {
        h = (g - b) / df;
        if (h < 0.f) h += 6.f;
    } else if (mx == g) {
        h = (b - r) / df + 2.f;
    } else {
        h = (r - g) / df + 4.f;
    }
    h *= (1.0f / 6.0f);  // [0,1)
}
__device__ __forceinline__ void hsv2rgb(float h, float s, float v, float& r, float& g, float& b) {
    const float h6 = (h - floorf(h)) * 6.f;
    const int i = (int)floorf(h6) % 6;
    const float f = h6 - floorf(h6);
    const float p = v * (1.f - s), q = v * (1.f - f * s), t = v * (1.f - (1.f - f) * s);
    switch (i) {
        case 0: r = v; g = t; b = p; break;
        case 1: r = q; g = v; b = p; break;
        case 2: r = p; g = v; b = t; break;
        case 3: r = p; g = q; b = v; break;
        case 4: r = t; g = p; b = v; break;
        default: r = v; g = p; b = q; break;
    }
}

// Per-image augmentation parameters from raw uniform draws (the arithmetic of ScrAugment.sample_params, agents/scr.py, one thread
// per image): 10 crop attempts of (area, log-ratio), first fit wins, centre-crop fallback; position, flip, jitter factors, order, gray.
struct AugCfg {
    float s0, ds, lr0, dlr;            // scale lower bound / width, log-ratio lower bound / width
    float b, c, s, hue, p_jit, p_gray;
    float fb_w, fb_h;                  // fallback crop (whole image with the aspect ratio clamped)
    float j0[4], j1[4];                // jitter factor = j0 + j1 * u  (1-b, 2b; 1-c, 2c; 1-s, 2s; -hue, 2 hue)
};
__global__ void __launch_bounds__(64) aug_params_kernel(const float* __restrict__ u, int n, int h, int w, AugCfg cfg,
                                                        float* __restrict__ params) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float* ui = u + (int64_t)i * OCL_AUG_NUNIFORM;
    const float H = (float)h, W = (float)w;
    float cw = 0.f, ch = 0.f;
    bool found = false;
    for (int t = 0; t < 10; ++t) {
        const float area = __fmul_rn(__fmul_rn(__fadd_rn(cfg.s0, __fmul_rn(cfg.ds, ui[t])), H), W);
        const float r = expf(__fadd_rn(cfg.lr0, __fmul_rn(cfg.dlr, ui[10 + t])));
        const float cwt = rintf(sqrtf(__fmul_rn(area, r)));
        const float cht = rintf(sqrtf(area / r));
        const bool fit = cwt > 0.f && cwt <= W && cht > 0.f && cht <= H;
        if (fit && !found) {
            found = true;
            cw = cwt;
            ch = cht;
        }
    }
    const float* e = ui + 20;
    float y0, x0;
    if (found) {
        y0 = fminf(floorf(__fmul_rn(e[0], H - ch + 1.f)), H - 1.f);
        x0 = fminf(floorf(__fmul_rn(e[1], W - cw + 1.f)), W - 1.f);
    } else {
        cw = cfg.fb_w;
        ch = cfg.fb_h;
        y0 = floorf((H - ch) / 2.f);
        x0 = floorf((W - cw) / 2.f);
    }
    float* p = params + (int64_t)i * OCL_AUG_NPARAM;
    p[0] = y0; p[1] = x0; p[2] = ch; p[3] = cw;
    p[4] = e[2] < 0.5f ? 1.f : 0.f;
    p[5] = e[3] < cfg.p_jit ? 1.f : 0.f;
#pragma unroll
    for (int k = 0; k < 4; ++k) p[6 + k] = __fadd_rn(cfg.j0[k], __fmul_rn(cfg.j1[k], e[4 + k]));
    p[10] = fminf(fmaxf(floorf(__fmul_rn(e[8], 24.f)), 0.f), 23.f);
    p[11] = e[9] < cfg.p_gray ? 1.f : 0.f;
}

__global__ void __launch_bounds__(256) augment_kernel(const float* __restrict__ x, float* __restrict__ out, int h, int w,
                                                      const float* __restrict__ params) {
    const int n = blockIdx.y;
    const int pix = blockIdx.x * blockDim.x + threadIdx.x;
    if (pix >= h * w) return;
    const float* pr = params + (int64_t)n * OCL_AUG_NPARAM;
    const float y0 = pr[0], x0 = pr[1], ch = pr[2], cw = pr[3];
    const bool flip = pr[4] > 0.5f, jit = pr[5] > 0.5f, gray = pr[11] > 0.5f;
    const int oy = pix / w, oxr = pix - oy * w;
    const int ox = flip ? (w - 1 - oxr) : oxr;
    // bilinear crop+resize, half-pixel centres, edge clamp
    float sy = y0 + ((float)oy + 0.5f) * (ch / (float)h) - 0.5f;
    float sx = x0 + ((float)ox + 0.5f) * (cw / (float)w) - 0.5f;
    sy = fminf(fmaxf(sy, 0.f), (float)(h - 1));
    sx = fminf(fmaxf(sx, 0.f), (float)(w - 1));
    const int iy0 = (int)floorf(sy), ix0 = (int)floorf(sx);
    const int iy1 = min(iy0 + 1, h - 1), ix1 = min(ix0 + 1, w - 1);
    const float fy = sy - (float)iy0, fx = sx - (float)ix0;
    const float* img = x + (int64_t)n * 3 * h * w;
    float c[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float* p = img + (int64_t)k * h * w;
        const float a = p[iy0 * w + ix0], b = p[iy0 * w + ix1], cc = p[iy1 * w + ix0], dd = p[iy1 * w + ix1];
        const float top = a + (b - a) * fx, bot = cc + (dd - cc) * fx;
        c[k] = top + (bot - top) * fy;
    }
    if (jit) {
        // the 24 permutations of {0:brightness,1:contrast,2:saturation,3:hue} in lexicographic order
        int ord = (int)pr[10];
        unsigned avail = 0x3210u;   // the operations still to run, one nibble each, in ascending order (registers: an indexed array would live in scratch)
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const int f = s == 0 ? 6 : s == 1 ? 2 : 1;
            const int q = ord / f;
            ord -= q * f;
            const int op = (int)((avail >> (4 * q)) & 15u);
            avail = (avail & ((1u << (4 * q)) - 1u)) | ((avail >> (4 * (q + 1))) << (4 * q));   // drop nibble q
            if (op == 0) {  // additive brightness (kornia 0.4-style): x + (f - 1)
                const float d = pr[6] - 1.f;
                c[0] = clamp01(c[0] + d); c[1] = clamp01(c[1] + d); c[2] = clamp01(c[2] + d);
            } else if (op == 1) {  // multiplicative contrast
                const float f = pr[7];
                c[0] = clamp01(c[0] * f); c[1] = clamp01(c[1] * f); c[2] = clamp01(c[2] * f);
            } else if (op == 2) {
                float hh, ss, vv;
                rgb2hsv(c[0], c[1], c[2], hh, ss, vv);
                ss = clamp01(ss * pr[8]);
                hsv2rgb(hh, ss, vv, c[0], c[1], c[2]);
            } else {
                float hh, ss, vv;
                rgb2hsv(c[0], c[1], c[2], hh, ss, vv);
                hh = hh + pr[9];
                hsv2rgb(hh, ss, vv, c[0], c[1], c[2]);
            }
        }
    }
    if (gray) {
        const float g = 0.299f * c[0] + 0.587f * c[1] + 0.114f * c[2];
        c[0] = c[1] = c[2] = g;
    }
    float* o = out + (int64_t)n * 3 * h * w;
    o[oy * w + oxr] = c[0];
    o[(int64_t)h * w + oy * w + oxr] = c[1];
    o[(int64_t)2 * h * w + oy * w + oxr] = c[2];
}

int ocl_scr_augment(const float* x, float* out, int n, int h, int w, const float* params, void* stream) {
    OCL_REQUIRE(n >= 0 && h > 0 && w > 0, "augment: bad shape");
    const SPlan pl = plan_augment(n, h, w);
    OCL_REQUIRE(pl.path != OCL_PATH_AUGMENT_REFUSED, "augment: n=%d h=%d w=%d too large (n <= 65535, h*w <= 2^31-256)", n, h, w);
    if (n == 0) return OCL_OK;
    OCL_REQUIRE(x && out && params && x != out, "augment: null pointer or in-place");
    hipStream_t s = (hipStream_t)stream;
    ProfScope ps(PROF_BN, s);
    hipLaunchKernelGGL(augment_kernel, dim3(pl.grid_x, pl.grid_y), dim3(pl.block), 0, s, x, out, h, w, params);
    OCL_LAUNCH_CHECK();
    return OCL_OK;
}

int ocl_scr_augment_uniform(const float* x, float* out, int n, int h, int w, const float* u, const double* cfg12, float* params,
                            void* stream) {
    OCL_REQUIRE(n >= 0 && h > 0 && w > 0, "augment: bad shape");
    const SPlan pl = plan_augment(n, h, w), pp = plan_aug_params(n);
    OCL_REQUIRE(pl.path != OCL_PATH_AUGMENT_REFUSED, "augment: n=%d h=%d w=%d too large (n <= 65535, h*w <= 2^31-256)", n, h, w);
    if (n == 0) return OCL_OK;
    OCL_REQUIRE(x && out && u && cfg12 && params && x != out, "augment: null pointer or in-place");
    AugCfg cfg;
    // derived constants in double, rounded once (what the host arithmetic does with Python floats applied to fp32 tensors)
    cfg.s0 = (float)cfg12[0]; cfg.ds = (float)(cfg12[1] - cfg12[0]);
    cfg.lr0 = (float)log(cfg12[2]); cfg.dlr = (float)(log(cfg12[3]) - log(cfg12[2]));
    cfg.b = (float)cfg12[4]; cfg.c = (float)cfg12[5]; cfg.s = (float)cfg12[6]; cfg.hue = (float)cfg12[7];
    cfg.p_jit = (float)cfg12[8]; cfg.p_gray = (float)cfg12[9];
    cfg.fb_w = (float)cfg12[10]; cfg.fb_h = (float)cfg12[11];
    for (int k = 0; k < 3; ++k) {
        cfg.j0[k] = (float)(1.0 - cfg12[4 + k]);
        cfg.j1[k] = (float)(2.0 * cfg12[4 + k]);
    }
    cfg.j0[3] = (float)(-cfg12[7]);
    cfg.j1[3] = (float)(2.0 * cfg12[7]);
    hipStream_t s = (hipStream_t)stream;
    ProfScope ps(PROF_BN, s);
    hipLaunchKernelGGL(aug_params_kernel, dim3(pp.grid_x), dim3(pp.block), 0, s, u, n, h, w, cfg, params);
    OCL_LAUNCH_CHECK();
    hipLaunchKernelGGL(augment_kernel, dim3(pl.grid_x, pl.grid_y), dim3(pl.block), 0, s, x, out, h, w, (const float*)params);
    OCL_LAUNCH_CHECK();
    return OCL_OK;
}
