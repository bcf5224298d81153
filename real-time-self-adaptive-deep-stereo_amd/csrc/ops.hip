// ops.hip -- the bandwidth-bound glue of the MADNet hot path for gfx950: feature warping,
// TF1-legacy bilinear resize (+scale/relu/crop fusions), reflect padding, the photometric
// SSIM+L1 reprojection loss with its disparity gradient, validation metrics, momentum update.
// Every kernel is a coalesced NHWC stream with 16-byte accesses where the layout allows;
// reductions are two-stage (wave shuffles -> per-block partial -> one finishing block) so the
// results are deterministic.
#include "mh_common.h"

namespace {

__device__ __forceinline__ float clampf(float v, float lo, float hi) { return fminf(fmaxf(v, lo), hi); }

// ------------------------------------------------------------------------------------------
// MadNet._linear_warping (Nets/MadNet.py:400-436) with coords from _build_indeces (:378-397)
// ------------------------------------------------------------------------------------------
struct WarpArgs {
    const float* img; const float* u; const float* g; float* out; float* dimg; float* du;
    int img_ld, out_ld, g_ld, dimg_ld, acc_u;
    int B, H, W, C;
    int64_t total;
};

__global__ __launch_bounds__(256) void warp_fwd_kernel(WarpArgs p) {
    const int C4 = p.C >> 2;
    for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < p.total; q += (int64_t)gridDim.x * 256) {
        const int c4 = (int)(q % C4);
        const int64_t pix = q / C4;
        const int x = (int)(pix % p.W);
        const int64_t rowbase = pix - x;
        const float cx = (float)x + p.u[pix];
        const float x0 = floorf(cx), x1 = x0 + 1.0f;
        const float xmax = (float)(p.W - 1);
        const float x0s = clampf(x0, 0.f, xmax), x1s = clampf(x1, 0.f, xmax);
        const float w0 = (x1 - cx) * (x0 == x0s ? 1.f : 0.f);
        const float w1 = (cx - x0) * (x1 == x1s ? 1.f : 0.f);
        const float4 a = *reinterpret_cast<const float4*>(p.img + (rowbase + (int)x0s) * p.img_ld + c4 * 4);
        const float4 b = *reinterpret_cast<const float4*>(p.img + (rowbase + (int)x1s) * p.img_ld + c4 * 4);
        float4 o;
        o.x = w0 * a.x + w1 * b.x; o.y = w0 * a.y + w1 * b.y;
        o.z = w0 * a.z + w1 * b.z; o.w = w0 * a.w + w1 * b.w;
        *reinterpret_cast<float4*>(p.out + pix * p.out_ld + c4 * 4) = o;
    }
}

// one wave = 64 lanes = (64/LPP) pixels x LPP channel lanes; du reduced with shuffles.
template <int LPP>
__global__ __launch_bounds__(256) void warp_bwd_kernel(WarpArgs p) {
    const int C4 = p.C >> 2;
    constexpr int PPB = 256 / LPP;
    const int sub = threadIdx.x % LPP;
    const int64_t npix = (int64_t)p.B * p.H * p.W;
    const int64_t nit = (npix + PPB - 1) / PPB;
    for (int64_t it = blockIdx.x; it < nit; it += gridDim.x) {
        const int64_t pix = it * PPB + threadIdx.x / LPP;
        const bool live = pix < npix;
        const int64_t pp = live ? pix : 0;
        const int x = (int)(pp % p.W);
        const int64_t rowbase = pp - x;
        const float cx = (float)x + p.u[pp];
        const float x0 = floorf(cx), x1 = x0 + 1.0f;
        const float xmax = (float)(p.W - 1);
        const float x0s = clampf(x0, 0.f, xmax), x1s = clampf(x1, 0.f, xmax);
        const float m0 = (x0 == x0s) ? 1.f : 0.f, m1 = (x1 == x1s) ? 1.f : 0.f;
        const float w0 = (x1 - cx) * m0, w1 = (cx - x0) * m1;
        const int i0 = (int)x0s, i1 = (int)x1s;
        float dcx = 0.f;
        for (int c4 = sub; c4 < C4; c4 += LPP) {
            if (!live) continue;
            const float4 gv = *reinterpret_cast<const float4*>(p.g + pp * p.g_ld + c4 * 4);
            if (p.dimg) {
                float* d0 = p.dimg + (rowbase + i0) * p.dimg_ld + c4 * 4;
                float* d1 = p.dimg + (rowbase + i1) * p.dimg_ld + c4 * 4;
                if (w0 != 0.f) { mh_atomic_add(d0 + 0, w0 * gv.x); mh_atomic_add(d0 + 1, w0 * gv.y); mh_atomic_add(d0 + 2, w0 * gv.z); mh_atomic_add(d0 + 3, w0 * gv.w); }
                if (w1 != 0.f) { mh_atomic_add(d1 + 0, w1 * gv.x); mh_atomic_add(d1 + 1, w1 * gv.y); mh_atomic_add(d1 + 2, w1 * gv.z); mh_atomic_add(d1 + 3, w1 * gv.w); }
            }
            if (p.du) {
                const float4 a = *reinterpret_cast<const float4*>(p.img + (rowbase + i0) * p.img_ld + c4 * 4);
                const float4 b = *reinterpret_cast<const float4*>(p.img + (rowbase + i1) * p.img_ld + c4 * 4);
                dcx += gv.x * (m1 * b.x - m0 * a.x) + gv.y * (m1 * b.y - m0 * a.y) +
                       gv.z * (m1 * b.z - m0 * a.z) + gv.w * (m1 * b.w - m0 * a.w);
            }
        }
        if (p.du) {
#pragma unroll
            for (int o = LPP >> 1; o > 0; o >>= 1) dcx += __shfl_xor(dcx, o);
            if (live && sub == 0) p.du[pp] = p.acc_u ? p.du[pp] + dcx : dcx;
        }
    }
}

// ------------------------------------------------------------------------------------------
// TF1 legacy bilinear resize + scale / relu / crop fusions
// ------------------------------------------------------------------------------------------
struct ResizeArgs {
    const float* in; const float* g; float* out; float* din;
    int B, Hi, Wi, Hr, Wr, cy, cx, Ho, Wo, mode, accumulate;
    float mul, sy, sx;   // sy = (float)Hi/(float)Hr
};

__device__ __forceinline__ void interp1(int i, float scale, int n, int& lo, int& hi, float& t) {
    const float src = (float)i * scale;
    lo = (int)src;
    hi = min(lo + 1, n - 1);
    t = src - (float)lo;
}

// (no mul+add contraction in the interpolation arithmetic: the resize kernels and the fused level front end of corr.hip then
//  produce bit-identical values, and the CPU emulator build -- no fma on plain x86-64 -- matches the GPU)
__device__ __forceinline__ float bilerp(const float* img, int Wi, int y0, int y1, float ty, int x0, int x1, float tx,
                                        float mul, bool relu_in) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    float tl = img[(int64_t)y0 * Wi + x0], tr = img[(int64_t)y0 * Wi + x1];
    float bl = img[(int64_t)y1 * Wi + x0], br = img[(int64_t)y1 * Wi + x1];
    if (relu_in) {
        tl = fmaxf(tl * mul, 0.f); tr = fmaxf(tr * mul, 0.f);
        bl = fmaxf(bl * mul, 0.f); br = fmaxf(br * mul, 0.f);
    }
    const float top = tl + (tr - tl) * tx;
    const float bot = bl + (br - bl) * tx;
    return top + (bot - top) * ty;
}

__global__ __launch_bounds__(256) void resize_fwd_kernel(ResizeArgs p) {
    const int64_t total = (int64_t)p.B * p.Ho * p.Wo;
    for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < total; q += (int64_t)gridDim.x * 256) {
        const int x = (int)(q % p.Wo);
        const int64_t t2 = q / p.Wo;
        const int y = (int)(t2 % p.Ho);
        const int b = (int)(t2 / p.Ho);
        int y0, y1, x0, x1; float ty, tx;
        interp1(y + p.cy, p.sy, p.Hi, y0, y1, ty);
        interp1(x + p.cx, p.sx, p.Wi, x0, x1, tx);
        const float* img = p.in + (int64_t)b * p.Hi * p.Wi;
        float v = bilerp(img, p.Wi, y0, y1, ty, x0, x1, tx, p.mul, p.mode == 1);
        if (p.mode == 0) v *= p.mul;
        else if (p.mode == 2) v = fmaxf(v * p.mul, 0.f);
        p.out[q] = v;
    }
}

// gather form of ResizeBilinearGrad: one lane per INPUT pixel, loops the output pixels whose
// lower/upper source index hits it (exactly the forward's float index arithmetic).
// LPP lanes share one input pixel and split the candidate output ROWS (an up-scaling by 4 gives an input pixel ~8 x 8 candidate
// output pixels, each needing the forward's bilinear taps again for the relu mask of mode 2: serial per lane that was 21 us for the
// 96x320 -> 375x1242 head at the start of the backward pass); partial sums meet in a shuffle butterfly.
template <int LPP>
__global__ __launch_bounds__(256) void resize_bwd_kernel(ResizeArgs p) {
    const int64_t total = (int64_t)p.B * p.Hi * p.Wi;
    const float isy = 1.0f / p.sy, isx = 1.0f / p.sx;
    const int sub = LPP > 1 ? (int)(threadIdx.x % LPP) : 0;
    const int64_t nit = (total * LPP + 255) / 256;              // every lane of a wave runs the same trip count (shuffles below)
    for (int64_t it = blockIdx.x; it < nit; it += gridDim.x) {
        const int64_t q0 = (it * 256 + threadIdx.x) / LPP;
        const bool live = q0 < total;
        const int64_t q = live ? q0 : 0;
        const int sx = (int)(q % p.Wi);
        const int64_t t2 = q / p.Wi;
        const int sy = (int)(t2 % p.Hi);
        const int b = (int)(t2 / p.Hi);
        const float* img = p.in + (int64_t)b * p.Hi * p.Wi;
        const float* gimg = p.g + (int64_t)b * p.Ho * p.Wo;
        const int ya = max(p.cy, (int)floorf((float)(sy - 1) * isy) - 1);
        const int yb = min(p.cy + p.Ho - 1, (int)ceilf((float)(sy + 1) * isy) + 1);
        const int xa = max(p.cx, (int)floorf((float)(sx - 1) * isx) - 1);
        const int xb = min(p.cx + p.Wo - 1, (int)ceilf((float)(sx + 1) * isx) + 1);
        float acc = 0.f;
        for (int Y = ya + sub; Y <= yb && live; Y += LPP) {
            int y0, y1; float ty;
            interp1(Y, p.sy, p.Hi, y0, y1, ty);
            const float wy = (y0 == sy ? 1.0f - ty : 0.f) + (y1 == sy ? ty : 0.f);
            if (wy == 0.f) continue;
            for (int X = xa; X <= xb; ++X) {
                int x0, x1; float tx;
                interp1(X, p.sx, p.Wi, x0, x1, tx);
                const float wx = (x0 == sx ? 1.0f - tx : 0.f) + (x1 == sx ? tx : 0.f);
                if (wx == 0.f) continue;
                float gv = gimg[(int64_t)(Y - p.cy) * p.Wo + (X - p.cx)];
                if (p.mode == 2) {
                    const float z = bilerp(img, p.Wi, y0, y1, ty, x0, x1, tx, p.mul, false) * p.mul;
                    if (!(z > 0.f)) gv = 0.f;
                }
                acc += gv * wy * wx;
            }
        }
#pragma unroll
        for (int o = LPP >> 1; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
        if (live && sub == 0) {
            acc *= p.mul;
            if (p.mode == 1 && !(img[(int64_t)sy * p.Wi + sx] * p.mul > 0.f)) acc = 0.f;
            p.din[q] = p.accumulate ? p.din[q] + acc : acc;
        }
    }
}

// ------------------------------------------------------------------------------------------
// backward front end of a disparity head in ONE launch (mh_head_bwd): the head's output gradient dV is assembled from what feeds it --
//   kind 0: the coordinate gradient du of the next finer level through the gradient of the x2 legacy resize (u = resize(V) * 20 / 2^k,
//           Nets/MadNet.py:274): exactly resize_bwd_kernel<1>'s gather, same summation order;
//   kind 1: two per-pixel addends with their own pixel strides (level 2: dfinal and the disparity channel of the context input's gradient)
// -- written out (fp32 + the bf16 shadow the streamed filter gradient of the head reads), and pushed through the head's 3x3 Cin -> 1 conv
// backwards (conv_k1_dgrad_kernel's arithmetic) with the leaky mask of the layer below, again with the shadow.  Two launches (three at
// level 2) of ~7 us each on the critical chain before.  A workgroup owns 4 x 32 head pixels; dV of the tile + a one-pixel halo goes through LDS.
// ------------------------------------------------------------------------------------------
struct HeadBwdArgs {
    ResizeArgs rz;                   // kind 0: rz.g = du (fine), Hi x Wi = the head's size
    const float* a1; const float* a2; int a1_ld, a2_ld;      // kind 1
    float* dV; unsigned short* dV_sh; int dV_sh_ld;
    const float* w; float* dx; const float* mask_ref; unsigned short* dx_sh;
    int N, dx_ld, mask_ld, dx_sh_ld, acc_dx, kind;
    float mask_alpha;
    int tiles_x, tiles_y;
};
#define HB_TH 4
#define HB_TW 32
__device__ __forceinline__ float head_dv_from_du(const ResizeArgs& p, int b, int sy, int sx, bool exact2) {
    const float* gimg = p.g + (int64_t)b * p.Ho * p.Wo;
    if (exact2) {
        // Hr = 2 Hi, no crop: fine row Y = 2 sy sits on the coarse row (weight 1), its neighbours half way (0.5; the last fine row clamps
        // onto the last coarse row: 1).  Same candidates, weights and order as the general walk below -- bit-identical, without its index search.
        // (the nine candidates are loaded unconditionally from clamped addresses and the out-of-range ones dropped by a select: loads inside `continue`
        //  branches were nine memory round trips one after the other -- round 4)
        float v[9], wgt[9];
        bool ok[9];
#pragma unroll
        for (int dy = -1; dy <= 1; ++dy) {
            const int Y = 2 * sy + dy;
            const bool oky = (unsigned)Y < (unsigned)p.Ho;
            const int Yc = oky ? Y : 2 * sy;
            const float wy = dy == 0 ? 1.0f : ((dy == 1 && sy == p.Hi - 1) ? 1.0f : 0.5f);
#pragma unroll
            for (int dx = -1; dx <= 1; ++dx) {
                const int X = 2 * sx + dx;
                const bool okx = (unsigned)X < (unsigned)p.Wo;
                const int Xc = okx ? X : 2 * sx;
                const float wx = dx == 0 ? 1.0f : ((dx == 1 && sx == p.Wi - 1) ? 1.0f : 0.5f);
                const int k = (dy + 1) * 3 + dx + 1;
                v[k] = gimg[(int64_t)Yc * p.Wo + Xc] * wy;
                wgt[k] = wx; ok[k] = oky && okx;
            }
        }
        float acc = 0.f;
#pragma unroll
        for (int k = 0; k < 9; ++k) acc += ok[k] ? v[k] * wgt[k] : 0.f;
        return acc * p.mul;
    }
    const float isy = 1.0f / p.sy, isx = 1.0f / p.sx;
    const int ya = max(p.cy, (int)floorf((float)(sy - 1) * isy) - 1);
    const int yb = min(p.cy + p.Ho - 1, (int)ceilf((float)(sy + 1) * isy) + 1);
    const int xa = max(p.cx, (int)floorf((float)(sx - 1) * isx) - 1);
    const int xb = min(p.cx + p.Wo - 1, (int)ceilf((float)(sx + 1) * isx) + 1);
    float acc = 0.f;
    for (int Y = ya; Y <= yb; ++Y) {
        int y0, y1; float ty;
        interp1(Y, p.sy, p.Hi, y0, y1, ty);
        const float wy = (y0 == sy ? 1.0f - ty : 0.f) + (y1 == sy ? ty : 0.f);
        if (wy == 0.f) continue;
        for (int X = xa; X <= xb; ++X) {
            int x0, x1; float tx;
            interp1(X, p.sx, p.Wi, x0, x1, tx);
            const float wx = (x0 == sx ? 1.0f - tx : 0.f) + (x1 == sx ? tx : 0.f);
            if (wx == 0.f) continue;
            acc += gimg[(int64_t)(Y - p.cy) * p.Wo + (X - p.cx)] * wy * wx;
        }
    }
    return acc * p.mul;
}
__global__ __launch_bounds__(256) void head_bwd_kernel(HeadBwdArgs p) {
    __shared__ float sV[(HB_TH + 2) * (HB_TW + 2)];
    __shared__ __attribute__((aligned(16))) float sW[9 * 64];
    const int tid = threadIdx.x;
    const int H = p.rz.Hi, W = p.rz.Wi;
    const int tx = blockIdx.x % p.tiles_x;
    const int t2 = blockIdx.x / p.tiles_x;
    const int ty = t2 % p.tiles_y, b = t2 / p.tiles_y;
    const int y0 = ty * HB_TH, x0 = tx * HB_TW;
    const bool exact2 = p.kind == 0 && p.rz.Hr == 2 * H && p.rz.Wr == 2 * W && p.rz.cy == 0 && p.rz.cx == 0 && p.rz.Ho == p.rz.Hr && p.rz.Wo == p.rz.Wr;
    for (int i = tid; i < 9 * p.N; i += 256) sW[i] = p.w[i];
    if (tid < (HB_TH + 2) * (HB_TW + 2)) {
        const int ly = tid / (HB_TW + 2), lx = tid - ly * (HB_TW + 2);
        const int y = y0 - 1 + ly, x = x0 - 1 + lx;
        float v = 0.f;
        if ((unsigned)y < (unsigned)H && (unsigned)x < (unsigned)W) {
            const int64_t pix = ((int64_t)b * H + y) * W + x;
            if (p.kind == 0) v = head_dv_from_du(p.rz, b, y, x, exact2);
            else v = (p.a1 ? p.a1[pix * p.a1_ld] : 0.f) + (p.a2 ? p.a2[pix * p.a2_ld] : 0.f);
            if (ly >= 1 && ly <= HB_TH && lx >= 1 && lx <= HB_TW) {
                p.dV[pix] = v;
                if (p.dV_sh) p.dV_sh[pix * p.dV_sh_ld] = (unsigned short)mh_pack_bf16(v, 0.f);
            }
        }
        sV[tid] = v;
    }
    __syncthreads();
    // dx[y][x][n] = mask(sum_taps dV[y + 1 - ky][x + 1 - kx] * w[ky][kx][n]) (+ old)
    const int G4 = p.N >> 2;
    if (G4 <= 16 && (p.acc_dx || p.mask_ref)) {
        // up to 8 items per thread: the old map / the mask of every item requested before the first is consumed (a load per loop iteration behind a store
        // to the same buffer cannot be hoisted by the compiler: four dependent round trips for a 32-channel head)
        constexpr int MAXIT = HB_TH * HB_TW * 16 / 256;
        float4 oldv[MAXIT], mkv[MAXIT];
#pragma unroll
        for (int it = 0; it < MAXIT; ++it) {
            const int i = tid + it * 256;
            const int g = i % G4, px = i / G4;
            const int iy = px / HB_TW, ix = px - iy * HB_TW;
            const int y = y0 + iy, x = x0 + ix;
            const bool live = i < HB_TH * HB_TW * G4 && y < H && x < W;
            const int64_t m = ((int64_t)b * H + (live ? y : y0)) * W + (live ? x : x0);
            oldv[it] = (live && p.acc_dx) ? *reinterpret_cast<const float4*>(p.dx + m * p.dx_ld + g * 4) : make_float4(0.f, 0.f, 0.f, 0.f);
            mkv[it] = (live && p.mask_ref) ? *reinterpret_cast<const float4*>(p.mask_ref + m * p.mask_ld + g * 4) : make_float4(1.f, 1.f, 1.f, 1.f);
        }
#pragma unroll
        for (int it = 0; it < MAXIT; ++it) {
            const int i = tid + it * 256;
            if (i >= HB_TH * HB_TW * G4) break;
            const int g = i % G4, px = i / G4;
            const int iy = px / HB_TW, ix = px - iy * HB_TW;
            const int y = y0 + iy, x = x0 + ix;
            if (y >= H || x >= W) continue;
            const int n = g * 4;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
            for (int t = 0; t < 9; ++t) {
                const int ky = t / 3, kx = t - ky * 3;
                const float z = sV[(iy + 2 - ky) * (HB_TW + 2) + ix + 2 - kx];
                const float4 w = *reinterpret_cast<const float4*>(sW + t * p.N + n);
                v.x += z * w.x; v.y += z * w.y; v.z += z * w.z; v.w += z * w.w;
            }
            const int64_t m = ((int64_t)b * H + y) * W + x;
            float* dst = p.dx + m * p.dx_ld + n;
            if (p.acc_dx) { const float4 o = oldv[it]; v.x += o.x; v.y += o.y; v.z += o.z; v.w += o.w; }
            if (p.mask_ref) {
                const float4 mk = mkv[it];
                v.x *= mk.x > 0.f ? 1.0f : p.mask_alpha; v.y *= mk.y > 0.f ? 1.0f : p.mask_alpha;
                v.z *= mk.z > 0.f ? 1.0f : p.mask_alpha; v.w *= mk.w > 0.f ? 1.0f : p.mask_alpha;
            }
            *reinterpret_cast<float4*>(dst) = v;
            if (p.dx_sh) *reinterpret_cast<uint2*>(p.dx_sh + m * p.dx_sh_ld + n) = make_uint2(mh_pack_bf16(v.x, v.y), mh_pack_bf16(v.z, v.w));
        }
        return;
    }
    for (int i = tid; i < HB_TH * HB_TW * G4; i += 256) {
        const int g = i % G4, px = i / G4;
        const int iy = px / HB_TW, ix = px - iy * HB_TW;
        const int y = y0 + iy, x = x0 + ix;
        if (y >= H || x >= W) continue;
        const int n = g * 4;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int t = 0; t < 9; ++t) {
            const int ky = t / 3, kx = t - ky * 3;
            const float z = sV[(iy + 2 - ky) * (HB_TW + 2) + ix + 2 - kx];
            const float4 w = *reinterpret_cast<const float4*>(sW + t * p.N + n);
            v.x += z * w.x; v.y += z * w.y; v.z += z * w.z; v.w += z * w.w;
        }
        const int64_t m = ((int64_t)b * H + y) * W + x;
        float* dst = p.dx + m * p.dx_ld + n;
        if (p.acc_dx) { const float4 o = *reinterpret_cast<const float4*>(dst); v.x += o.x; v.y += o.y; v.z += o.z; v.w += o.w; }
        if (p.mask_ref) {
            const float4 mk = *reinterpret_cast<const float4*>(p.mask_ref + m * p.mask_ld + n);
            v.x *= mk.x > 0.f ? 1.0f : p.mask_alpha; v.y *= mk.y > 0.f ? 1.0f : p.mask_alpha;
            v.z *= mk.z > 0.f ? 1.0f : p.mask_alpha; v.w *= mk.w > 0.f ? 1.0f : p.mask_alpha;
        }
        *reinterpret_cast<float4*>(dst) = v;
        if (p.dx_sh) *reinterpret_cast<uint2*>(p.dx_sh + m * p.dx_sh_ld + n) = make_uint2(mh_pack_bf16(v.x, v.y), mh_pack_bf16(v.z, v.w));
    }
}

// ------------------------------------------------------------------------------------------
// multi-channel TF1-legacy bilinear resize of NHWC images (Stereo_Online_Adaptation.scale_tensor :22-23 ->
// preprocessing.rescale_image :269-273 on the 3-channel frames when --reprojectionScale != 1) and its gradient
// ------------------------------------------------------------------------------------------
struct ResizeImgArgs { const float* in; const float* g; float* out; float* din; int B, Hi, Wi, C, Ho, Wo; float sy, sx; };

__global__ __launch_bounds__(256) void resize_image_fwd_kernel(ResizeImgArgs p) {
    const int64_t total = (int64_t)p.B * p.Ho * p.Wo * p.C;
    for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < total; q += (int64_t)gridDim.x * 256) {
        const int c = (int)(q % p.C);
        int64_t t = q / p.C;
        const int x = (int)(t % p.Wo); t /= p.Wo;
        const int y = (int)(t % p.Ho);
        const int b = (int)(t / p.Ho);
        int y0, y1, x0, x1; float ty, tx;
        interp1(y, p.sy, p.Hi, y0, y1, ty);
        interp1(x, p.sx, p.Wi, x0, x1, tx);
        const float* img = p.in + (int64_t)b * p.Hi * p.Wi * p.C + c;
        const float tl = img[((int64_t)y0 * p.Wi + x0) * p.C], tr = img[((int64_t)y0 * p.Wi + x1) * p.C];
        const float bl = img[((int64_t)y1 * p.Wi + x0) * p.C], br = img[((int64_t)y1 * p.Wi + x1) * p.C];
        const float top = tl + (tr - tl) * tx, bot = bl + (br - bl) * tx;
        p.out[q] = top + (bot - top) * ty;
    }
}

// gather form (one lane per INPUT element), same index arithmetic as the forward
__global__ __launch_bounds__(256) void resize_image_bwd_kernel(ResizeImgArgs p) {
    const int64_t total = (int64_t)p.B * p.Hi * p.Wi * p.C;
    const float isy = 1.0f / p.sy, isx = 1.0f / p.sx;
    for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < total; q += (int64_t)gridDim.x * 256) {
        const int c = (int)(q % p.C);
        int64_t t = q / p.C;
        const int sx = (int)(t % p.Wi); t /= p.Wi;
        const int sy = (int)(t % p.Hi);
        const int b = (int)(t / p.Hi);
        const float* gimg = p.g + (int64_t)b * p.Ho * p.Wo * p.C + c;
        const int ya = max(0, (int)floorf((float)(sy - 1) * isy) - 1), yb = min(p.Ho - 1, (int)ceilf((float)(sy + 1) * isy) + 1);
        const int xa = max(0, (int)floorf((float)(sx - 1) * isx) - 1), xb = min(p.Wo - 1, (int)ceilf((float)(sx + 1) * isx) + 1);
        float acc = 0.f;
        for (int Y = ya; Y <= yb; ++Y) {
            int y0, y1; float ty;
            interp1(Y, p.sy, p.Hi, y0, y1, ty);
            const float wy = (y0 == sy ? 1.0f - ty : 0.f) + (y1 == sy ? ty : 0.f);
            if (wy == 0.f) continue;
            for (int X = xa; X <= xb; ++X) {
                int x0, x1; float tx;
                interp1(X, p.sx, p.Wi, x0, x1, tx);
                const float wx = (x0 == sx ? 1.0f - tx : 0.f) + (x1 == sx ? tx : 0.f);
                if (wx != 0.f) acc += gimg[((int64_t)Y * p.Wo + X) * p.C] * wy * wx;
            }
        }
        p.din[q] = acc;
    }
}

// ------------------------------------------------------------------------------------------
// preprocessing.bilinear_sampler (Data_utils/preprocessing.py:121-199), general form: out[b,y,x,:] = 4-tap bilinear sample
// of imgs[b] at coords[b,y,x] = (cx, cy).  Indices are CLAMPED to the border and the weights are NOT masked (the code's
// behaviour, not its docstring: SURVEY App. D.7); the flat gather index is computed in float32 like the reference (:170-187)
// and then cast.  Gradients: w.r.t. coords (d out / d cx = (wt_y0*(im10-im00) + wt_y1*(im11-im01)), likewise cy; floor has no
// gradient) and w.r.t. imgs (scatter, fp32 atomics into a pre-zeroed buffer).
// ------------------------------------------------------------------------------------------
struct SamplerArgs { const float* img; const float* coords; const float* g; float* out; float* dcoords; float* dimg;
                     int B, Hs, Ws, C, Ht, Wt; };

__device__ __forceinline__ void sampler_taps(const SamplerArgs& p, int b, float cx, float cy, int64_t (&idx)[4], float (&w)[4],
                                             float& wx0, float& wx1, float& wy0, float& wy1) {
    const float x0 = floorf(cx), x1 = x0 + 1.0f, y0 = floorf(cy), y1 = y0 + 1.0f;
    wx0 = x1 - cx; wx1 = cx - x0; wy0 = y1 - cy; wy1 = cy - y0;
    const float xm = (float)(p.Ws - 1), ym = (float)(p.Hs - 1);
    const float x0s = clampf(x0, 0.f, xm), x1s = clampf(x1, 0.f, xm), y0s = clampf(y0, 0.f, ym), y1s = clampf(y1, 0.f, ym);
    const float dim2 = (float)p.Ws, base = (float)b * (float)(p.Ws * p.Hs);
    const float by0 = base + y0s * dim2, by1 = base + y1s * dim2;
    idx[0] = (int64_t)(int)(x0s + by0); idx[1] = (int64_t)(int)(x0s + by1);        // im00, im01
    idx[2] = (int64_t)(int)(x1s + by0); idx[3] = (int64_t)(int)(x1s + by1);        // im10, im11
    w[0] = wx0 * wy0; w[1] = wx0 * wy1; w[2] = wx1 * wy0; w[3] = wx1 * wy1;
}

__global__ __launch_bounds__(256) void sampler_fwd_kernel(SamplerArgs p) {
    const int64_t total = (int64_t)p.B * p.Ht * p.Wt;
    for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < total; q += (int64_t)gridDim.x * 256) {
        const int b = (int)(q / ((int64_t)p.Ht * p.Wt));
        int64_t idx[4]; float w[4], wx0, wx1, wy0, wy1;
        sampler_taps(p, b, p.coords[q * 2], p.coords[q * 2 + 1], idx, w, wx0, wx1, wy0, wy1);
        for (int c = 0; c < p.C; ++c) {
            // tf.add_n([w00*im00, w01*im01, w10*im10, w11*im11]): left-to-right sum
            float v = w[0] * p.img[idx[0] * p.C + c];
            v += w[1] * p.img[idx[1] * p.C + c];
            v += w[2] * p.img[idx[2] * p.C + c];
            v += w[3] * p.img[idx[3] * p.C + c];
            p.out[q * p.C + c] = v;
        }
    }
}

__global__ __launch_bounds__(256) void sampler_bwd_kernel(SamplerArgs p) {
    const int64_t total = (int64_t)p.B * p.Ht * p.Wt;
    for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < total; q += (int64_t)gridDim.x * 256) {
        const int b = (int)(q / ((int64_t)p.Ht * p.Wt));
        int64_t idx[4]; float w[4], wx0, wx1, wy0, wy1;
        sampler_taps(p, b, p.coords[q * 2], p.coords[q * 2 + 1], idx, w, wx0, wx1, wy0, wy1);
        float gx = 0.f, gy = 0.f;
        for (int c = 0; c < p.C; ++c) {
            const float gv = p.g[q * p.C + c];
            const float i00 = p.img[idx[0] * p.C + c], i01 = p.img[idx[1] * p.C + c], i10 = p.img[idx[2] * p.C + c], i11 = p.img[idx[3] * p.C + c];
            // wt_x0 = x1 - cx (d/dcx = -1), wt_x1 = cx - x0 (+1); same for y
            gx += gv * (wy0 * (i10 - i00) + wy1 * (i11 - i01));
            gy += gv * (wx0 * (i01 - i00) + wx1 * (i11 - i10));
            if (p.dimg) {
                mh_atomic_add(p.dimg + idx[0] * p.C + c, gv * w[0]); mh_atomic_add(p.dimg + idx[1] * p.C + c, gv * w[1]);
                mh_atomic_add(p.dimg + idx[2] * p.C + c, gv * w[2]); mh_atomic_add(p.dimg + idx[3] * p.C + c, gv * w[3]);
            }
        }
        if (p.dcoords) { p.dcoords[q * 2] = gx; p.dcoords[q * 2 + 1] = gy; }
    }
}

// ------------------------------------------------------------------------------------------
// preprocessing.pad_image (REFLECT) + channel padding
// ------------------------------------------------------------------------------------------
struct PadArgs { const float* in; float* out; int B, H, W, C, Hp, Wp, pt, pl, out_ld; float div, sub; };

__global__ __launch_bounds__(256) void pad_reflect_kernel(PadArgs p) {
    const int64_t total = (int64_t)p.B * p.Hp * p.Wp;
    for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < total; q += (int64_t)gridDim.x * 256) {
        const int x = (int)(q % p.Wp);
        const int64_t t2 = q / p.Wp;
        const int y = (int)(t2 % p.Hp);
        const int b = (int)(t2 / p.Hp);
        int sy = y - p.pt, sx = x - p.pl;
        sy = sy < 0 ? -sy : (sy >= p.H ? 2 * (p.H - 1) - sy : sy);
        sx = sx < 0 ? -sx : (sx >= p.W ? 2 * (p.W - 1) - sx : sx);
        const float* src = p.in + (((int64_t)b * p.H + sy) * p.W + sx) * p.C;
        float* dst = p.out + q * p.out_ld;
        for (int c = 0; c < p.out_ld; ++c) dst[c] = c < p.C ? (p.div == 1.0f ? src[c] : src[c] / p.div) - p.sub : 0.f;
    }
}

// ------------------------------------------------------------------------------------------
// reprojection loss (mean_SSIM_L1 of warp_image(right, disp) vs left)
// ------------------------------------------------------------------------------------------
struct LossArgs {
    const float* left; const float* right; const float* disp;
    float* rep; float* drep; float* coef; float* part1; float* part2; float* result; float* ddisp;
    int B, H, W, nblk1, nblk2;
    float grad_scale;
};
// the masked loss only (a kernel argument of its own, behind the others: LossArgs and the unmasked kernels' argument offsets stay what they were):
// [B][H][W] masks, non-zero = valid; cnt[tile] = valid pixels, cnt[nblk1 + tile] = valid windows
struct LossMask { const uint8_t* valid_l; const uint8_t* valid_r; int* cnt; };

__device__ __forceinline__ float block_sum(float v, float* red) {
    v = mh_wave_sum(v);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    __syncthreads();
    if (lane == 0) red[wave] = v;
    __syncthreads();
    return red[0] + red[1] + red[2] + red[3];
}

// One launch for the maps and the gradient: a workgroup owns a 16 x 32 pixel tile and works through LDS on the tile + a 2-pixel halo
// (a pixel's gradient needs the SSIM coefficients of the <= 9 windows that contain it, a window needs the warped image at its 9 pixels):
//   A  warp right by the disparity at the 20 x 36 halo pixels (bilinear_sampler: clamped indices, un-masked weights; rows are integral
//      so only the y0 taps carry weight) -> LDS; d rep / d x for the tile's own pixels -> LDS; L1 partial sum over the tile's pixels;
//   B  SSIM over the 18 x 34 3x3 VALID windows that touch the tile -> per-window derivative coefficients in LDS
//        d map / d x_p = alpha + beta*y_p + gamma*x_p   for the 9 pixels p of the window
//      (windows outside the image: zeros); SSIM partial sum over the windows whose top-left corner is a pixel of the tile;
//   C  d loss / d disp[p] = - sum_ch (d loss / d rep[p,ch]) * drep[p,ch].
// (Three launches with the maps in HBM before: 39 us per step on the critical path at 375 x 1242; per-pixel arithmetic and summation order of
// the gradient unchanged.)
#define LT_H 16
#define LT_W 32
#define LT_HH (LT_H + 4)
#define LT_HW (LT_W + 4)
#define LT_WH (LT_H + 2)
#define LT_WW (LT_W + 2)

// ---- the masked loss (mh_reprojection_loss_masked): which pixels count ----
// Byte `idx` of a mask of n >= 4 bytes through its range-checked descriptor (idx = MH_OOB: 0).  The load is the dword that holds the byte; the last dword of a
// mask whose size is no multiple of 4 is read at n - 4, so no byte behind the mask is touched.
__device__ __forceinline__ unsigned loss_mask_byte(__amdgpu_buffer_rsrc_t rs, int idx, int n) {
    const int a = idx == MH_OOB ? MH_OOB : min(idx & ~3, n - 4);
    const unsigned w = __builtin_amdgcn_raw_buffer_load_b32(rs, a, 0, 0);
    return (w >> (((unsigned)(idx - a) & 3u) * 8u)) & 0xffu;
}
__device__ __forceinline__ bool loss_finite(float v) { return (__builtin_bit_cast(unsigned, v) & 0x7f800000u) != 0x7f800000u; }

// The count pass in front of the masked tile kernel, tiled like it: v(p) = valid_l[p] && valid_r at both taps of the warp && isfinite(disp[p]) on the tile + its
// halo -> LDS; cnt[tile] = valid pixels of the tile, cnt[nblk1 + tile] = windows whose top-left corner is a pixel of the tile and whose nine pixels are valid.
// Reads disp and the masks only; integer sums, so the order of the additions cannot change them.
__global__ __launch_bounds__(256) void loss_count_kernel(LossArgs p, int tiles_x, int tiles_y, LossMask m) {
    __shared__ unsigned char s_v[LT_HH * LT_HW];
    __shared__ int s_n[2];
    const int tid = threadIdx.x;
    const int tx = blockIdx.x % tiles_x;
    const int t2 = blockIdx.x / tiles_x;
    const int ty = t2 % tiles_y, b = t2 / tiles_y;
    const int y0t = ty * LT_H, x0t = tx * LT_W;
    const float xmax = (float)(p.W - 1);
    const int npx = p.B * p.H * p.W;
    const __amdgpu_buffer_rsrc_t rs_d = mh_make_rsrc(p.disp, (unsigned)npx * 4u);
    const __amdgpu_buffer_rsrc_t rs_vl = mh_make_rsrc(m.valid_l, (unsigned)npx);
    const __amdgpu_buffer_rsrc_t rs_vr = mh_make_rsrc(m.valid_r, (unsigned)npx);
    if (tid < 2) s_n[tid] = 0;
    for (int i = tid; i < LT_HH * LT_HW; i += 256) {
        const int ly = i / LT_HW, lx = i - ly * LT_HW;
        const int y = y0t - 2 + ly, x = x0t - 2 + lx;
        const bool inb = (unsigned)y < (unsigned)p.H && (unsigned)x < (unsigned)p.W;
        const int rb = (b * p.H + y) * p.W;
        const float d = mh_buf_load1(rs_d, inb ? (rb + x) * 4 : MH_OOB);
        const bool fin = inb && loss_finite(d);
        const float xf0 = floorf((float)x - d);
        const int i0 = (int)clampf(xf0, 0.f, xmax), i1 = (int)clampf(xf0 + 1.0f, 0.f, xmax);
        const unsigned ml = loss_mask_byte(rs_vl, inb ? rb + x : MH_OOB, npx);
        const unsigned m0 = loss_mask_byte(rs_vr, fin ? rb + i0 : MH_OOB, npx), m1 = loss_mask_byte(rs_vr, fin ? rb + i1 : MH_OOB, npx);
        s_v[i] = (ml != 0u && m0 != 0u && m1 != 0u) ? 1 : 0;
    }
    __syncthreads();
    const int Hw = p.H - 2, Ww = p.W - 2;
    int n1 = 0, n2 = 0;
    for (int i = tid; i < LT_H * LT_W; i += 256) {
        const int iy = i / LT_W, ix = i - iy * LT_W;
        const unsigned char* c = s_v + (iy + 2) * LT_HW + ix + 2;         // (pixels outside the image hold 0)
        n1 += c[0];
        if (y0t + iy < Hw && x0t + ix < Ww)
            n2 += c[0] & c[1] & c[2] & c[LT_HW] & c[LT_HW + 1] & c[LT_HW + 2] & c[2 * LT_HW] & c[2 * LT_HW + 1] & c[2 * LT_HW + 2];
    }
    if (n1) atomicAdd(s_n + 0, n1);
    if (n2) atomicAdd(s_n + 1, n2);
    __syncthreads();
    if (tid == 0) { m.cnt[blockIdx.x] = s_n[0]; m.cnt[p.nblk1 + blockIdx.x] = s_n[1]; }
}

// MASKED (mh_reprojection_loss_masked): a pixel that is not valid (loss_count_kernel's v) puts zeros into the LDS maps and nothing into the sums or the gradient --
// selected, never multiplied, so a NaN under it stays out; a window counts when its nine pixels do; the means run over the counts of loss_count_kernel.
template <bool MASKED>
__global__ __launch_bounds__(256) void loss_tile_kernel(LossArgs p, int tiles_x, int tiles_y, int with_grad, LossMask m) {
    __shared__ float red[4];
    __shared__ unsigned char s_v[MASKED ? LT_HH * LT_HW : 1];
    __shared__ int s_n[2];
    __shared__ float s_rep[LT_HH * LT_HW * 3];
    __shared__ float s_y[LT_HH * LT_HW * 3];
    __shared__ float s_drep[LT_H * LT_W * 3];
    __shared__ float s_coef[LT_WH * LT_WW * 9];
    const int tid = threadIdx.x;
    const int tx = blockIdx.x % tiles_x;
    const int t2 = blockIdx.x / tiles_x;
    const int ty = t2 % tiles_y, b = t2 / tiles_y;
    const int y0t = ty * LT_H, x0t = tx * LT_W;
    const float s = 1.0f / 256.0f;
    const float xmax = (float)(p.W - 1);
    if (MASKED && with_grad) {          // the counts of the whole batch, for the scale of the gradient: every workgroup sums the per-tile integers (L2 hits)
        if (tid < 2) s_n[tid] = 0;
        __syncthreads();
        int n1 = 0, n2 = 0;
        for (int i = tid; i < p.nblk1; i += 256) { n1 += m.cnt[i]; n2 += m.cnt[p.nblk1 + i]; }
        if (n1) atomicAdd(s_n + 0, n1);
        if (n2) atomicAdd(s_n + 1, n2);                                   // (published by the barriers of phases A and B)
    }
    // ---- A -------------------------------------------------------------------------------------
    // Round 5: the three halo pixels of a thread go through the phase TOGETHER -- three disparity loads in flight, then all 27 image loads (range-checked buffer
    // loads: a pixel outside the image = an out-of-range offset = zeros, no branch around a load).  The loop this replaces waited for disp, then for its nine
    // image values, once per pixel: six dependent memory round trips at the head of a launch that sits on the forward chain of every mode.
    float l1 = 0.f;
    {
        constexpr int NI = (LT_HH * LT_HW + 255) / 256;          // 3
        const unsigned npx = (unsigned)p.B * (unsigned)p.H * (unsigned)p.W;
        const __amdgpu_buffer_rsrc_t rs_d = mh_make_rsrc(p.disp, npx * 4u);
        const __amdgpu_buffer_rsrc_t rs_l = mh_make_rsrc(p.left, npx * 12u);
        const __amdgpu_buffer_rsrc_t rs_r = mh_make_rsrc(p.right, npx * 12u);
        const __amdgpu_buffer_rsrc_t rs_vl = mh_make_rsrc(m.valid_l, MASKED ? npx : 0u);
        const __amdgpu_buffer_rsrc_t rs_vr = mh_make_rsrc(m.valid_r, MASKED ? npx : 0u);
        unsigned mv[NI];
        int qv[NI], rbv[NI];
        bool inb[NI];
        float dv[NI];
#pragma unroll
        for (int u = 0; u < NI; ++u) {
            const int i = tid + u * 256;
            const int ly = i / LT_HW, lx = i - ly * LT_HW;
            const int y = y0t - 2 + ly, x = x0t - 2 + lx;
            inb[u] = i < LT_HH * LT_HW && (unsigned)y < (unsigned)p.H && (unsigned)x < (unsigned)p.W;
            rbv[u] = (b * p.H + y) * p.W;
            qv[u] = rbv[u] + x;
            dv[u] = mh_buf_load1(rs_d, inb[u] ? qv[u] * 4 : MH_OOB);
        }
        float av[NI][3], bv[NI][3], lv[NI][3], w0v[NI], w1v[NI];
#pragma unroll
        for (int u = 0; u < NI; ++u) {
            const int i = tid + u * 256;
            const int ly = i / LT_HW, lx = i - ly * LT_HW;
            const int x = x0t - 2 + lx;
            const float cx = (float)x - dv[u];
            const float xf0 = floorf(cx), xf1 = xf0 + 1.0f;
            w0v[u] = xf1 - cx; w1v[u] = cx - xf0;
            const int i0 = (int)clampf(xf0, 0.f, xmax), i1 = (int)clampf(xf1, 0.f, xmax);
            int o0 = (rbv[u] + i0) * 12, o1 = (rbv[u] + i1) * 12, ol = qv[u] * 12;
            MH_KEEP_VGPR(o0); MH_KEEP_VGPR(o1); MH_KEEP_VGPR(ol);
            if (MASKED) {                   // loss_count_kernel's v, from the same taps
                const bool fin = inb[u] && loss_finite(dv[u]);
                const unsigned ml = loss_mask_byte(rs_vl, inb[u] ? qv[u] : MH_OOB, (int)npx);
                const unsigned m0 = loss_mask_byte(rs_vr, fin ? rbv[u] + i0 : MH_OOB, (int)npx), m1 = loss_mask_byte(rs_vr, fin ? rbv[u] + i1 : MH_OOB, (int)npx);
                mv[u] = (ml != 0u && m0 != 0u && m1 != 0u) ? 1u : 0u;
            }
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                av[u][c] = mh_buf_load1(rs_r, inb[u] ? o0 + 4 * c : MH_OOB);
                bv[u][c] = mh_buf_load1(rs_r, inb[u] ? o1 + 4 * c : MH_OOB);
                lv[u][c] = mh_buf_load1(rs_l, inb[u] ? ol + 4 * c : MH_OOB);
            }
        }
#pragma unroll
        for (int u = 0; u < NI; ++u) {
            const int i = tid + u * 256;
            if (i >= LT_HH * LT_HW) break;
            const int ly = i / LT_HW, lx = i - ly * LT_HW;
            float r0v = 0.f, r1v = 0.f, r2v = 0.f, y0v = 0.f, y1v = 0.f, y2v = 0.f;
            if (MASKED ? mv[u] != 0u : inb[u]) {
                const float a0 = av[u][0] * s, a1 = av[u][1] * s, a2 = av[u][2] * s;
                const float b0 = bv[u][0] * s, b1 = bv[u][1] * s, b2 = bv[u][2] * s;
                const float w0 = w0v[u], w1 = w1v[u];
                r0v = w0 * a0 + w1 * b0; r1v = w0 * a1 + w1 * b1; r2v = w0 * a2 + w1 * b2;
                y0v = lv[u][0] * s; y1v = lv[u][1] * s; y2v = lv[u][2] * s;
                const int iy = ly - 2, ix = lx - 2;
                if ((unsigned)iy < (unsigned)LT_H && (unsigned)ix < (unsigned)LT_W) {
                    float* d = s_drep + (iy * LT_W + ix) * 3;
                    d[0] = b0 - a0; d[1] = b1 - a1; d[2] = b2 - a2;
                    l1 += fabsf(r0v - y0v) + fabsf(r1v - y1v) + fabsf(r2v - y2v);
                }
            }
            s_rep[i * 3 + 0] = r0v; s_rep[i * 3 + 1] = r1v; s_rep[i * 3 + 2] = r2v;
            s_y[i * 3 + 0] = y0v; s_y[i * 3 + 1] = y1v; s_y[i * 3 + 2] = y2v;
            if (MASKED) s_v[i] = (unsigned char)mv[u];
        }
    }
    __syncthreads();
    // ---- B -------------------------------------------------------------------------------------
    const int Hw = p.H - 2, Ww = p.W - 2;
    float ssum = 0.f;
    for (int i = tid; i < LT_WH * LT_WW; i += 256) {
        const int ly = i / LT_WW, lx = i - ly * LT_WW;
        const int wy = y0t - 2 + ly, wx = x0t - 2 + lx;              // window (wy, wx) = halo pixels (ly .. ly+2, lx .. lx+2)
        float co[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
        bool wok = (unsigned)wy < (unsigned)Hw && (unsigned)wx < (unsigned)Ww;
        if (MASKED) {
            const unsigned char* c = s_v + ly * LT_HW + lx;
            wok = wok && (c[0] & c[1] & c[2] & c[LT_HW] & c[LT_HW + 1] & c[LT_HW + 2] & c[2 * LT_HW] & c[2 * LT_HW + 1] & c[2 * LT_HW + 2]) != 0;
        }
        if (wok) {
            const float C1 = 0.01f * 0.01f, C2 = 0.03f * 0.03f;
            float sx[3] = {0, 0, 0}, sy[3] = {0, 0, 0}, sxx[3] = {0, 0, 0}, syy[3] = {0, 0, 0}, sxy[3] = {0, 0, 0};
            for (int dy = 0; dy < 3; ++dy)
                for (int dx = 0; dx < 3; ++dx) {
                    const int h = ((ly + dy) * LT_HW + lx + dx) * 3;
#pragma unroll
                    for (int c = 0; c < 3; ++c) {
                        const float xv = s_rep[h + c], yv = s_y[h + c];
                        sx[c] += xv; sy[c] += yv; sxx[c] += xv * xv; syy[c] += yv * yv; sxy[c] += xv * yv;
                    }
                }
            const bool own = ly >= 2 && lx >= 2 && ly < 2 + LT_H && lx < 2 + LT_W;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float inv9 = 1.0f / 9.0f;
                const float mx = sx[c] * inv9, my = sy[c] * inv9;
                const float vx = sxx[c] * inv9 - mx * mx, vy = syy[c] * inv9 - my * my, vxy = sxy[c] * inv9 - mx * my;
                const float n1 = 2.f * mx * my + C1, n2 = 2.f * vxy + C2;
                const float d1 = mx * mx + my * my + C1, d2 = vx + vy + C2;
                const float S = (n1 * n2) / (d1 * d2);
                const float mraw = (1.0f - S) * 0.5f;
                if (own) ssum += clampf(mraw, 0.f, 1.f);
                // tf.clip_by_value passes the gradient iff 0 <= x <= 1 ; d map = -0.5 dS
                const float pass = (mraw >= 0.f && mraw <= 1.f) ? -0.5f * (2.0f / 9.0f) : 0.f;
                const float idd = 1.0f / (d1 * d2);
                const float beta = n1 * idd;
                const float gamma = -S / d2;
                const float alpha = (my * n2 - n1 * my) * idd - S * (mx * d2 - d1 * mx) * idd;
                co[c * 3 + 0] = pass * alpha; co[c * 3 + 1] = pass * beta; co[c * 3 + 2] = pass * gamma;
            }
        }
#pragma unroll
        for (int k = 0; k < 9; ++k) s_coef[i * 9 + k] = co[k];
    }
    const float tot1 = block_sum(l1, red);          // (its barriers also publish s_coef)
    const float tot2 = block_sum(ssum, red);
    if (tid == 0) { p.part1[blockIdx.x] = tot1; p.part2[blockIdx.x] = tot2; }
    if (!with_grad) return;
    // ---- C -------------------------------------------------------------------------------------
    // (MASKED: the counts are integers, so below 2^24 of them these are the unmasked factors of an all-ones mask; an empty set has no term)
    const float k_ssim = MASKED ? (s_n[1] > 0 ? 0.85f / ((float)s_n[1] * 3.0f) : 0.f) : 0.85f / ((float)p.B * (float)Hw * (float)Ww * 3.0f);
    const float k_l1 = MASKED ? (s_n[0] > 0 ? 0.15f / ((float)s_n[0] * 3.0f) : 0.f) : 0.15f / ((float)p.B * (float)p.H * (float)p.W * 3.0f);
    for (int i = tid; i < LT_H * LT_W; i += 256) {
        const int iy = i / LT_W, ix = i - iy * LT_W;
        const int y = y0t + iy, x = x0t + ix;
        if (y >= p.H || x >= p.W) continue;
        float A[3] = {0, 0, 0}, Bc[3] = {0, 0, 0}, Gc[3] = {0, 0, 0};
        // windows (y-2 .. y, x-2 .. x) = local windows (iy .. iy+2, ix .. ix+2); the ones outside the image hold zeros
        for (int dy = 0; dy < 3; ++dy)
            for (int dx = 0; dx < 3; ++dx) {
                const float* cp = s_coef + ((iy + dy) * LT_WW + ix + dx) * 9;
                A[0] += cp[0]; Bc[0] += cp[1]; Gc[0] += cp[2];
                A[1] += cp[3]; Bc[1] += cp[4]; Gc[1] += cp[5];
                A[2] += cp[6]; Bc[2] += cp[7]; Gc[2] += cp[8];
            }
        const int h = ((iy + 2) * LT_HW + ix + 2) * 3;
        float gd = 0.f;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float xv = s_rep[h + c], yv = s_y[h + c];
            const float diff = xv - yv;
            const float sgn = diff > 0.f ? 1.f : (diff < 0.f ? -1.f : 0.f);
            const float grep = k_ssim * (A[c] + Bc[c] * yv + Gc[c] * xv) + k_l1 * sgn;
            gd -= grep * s_drep[i * 3 + c];
        }
        p.ddisp[((int64_t)b * p.H + y) * p.W + x] = (MASKED && !s_v[(iy + 2) * LT_HW + ix + 2]) ? 0.f : gd * p.grad_scale;
    }
}

// MASKED: the means run over the counts of loss_count_kernel (exact in float64); a term whose count is 0 is 0
template <bool MASKED>
__global__ __launch_bounds__(256) void loss_final_kernel(LossArgs p, LossMask m) {
    __shared__ double red[256];
    double a = 0.0, b = 0.0;
    double c1 = 0.0, c2 = 0.0;
    if (MASKED) {
        for (int i = threadIdx.x; i < p.nblk1; i += 256) { c1 += (double)m.cnt[i]; c2 += (double)m.cnt[p.nblk1 + i]; }
        red[threadIdx.x] = c1; __syncthreads();
        for (int o = 128; o > 0; o >>= 1) { if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o]; __syncthreads(); }
        c1 = red[0]; __syncthreads();
        red[threadIdx.x] = c2; __syncthreads();
        for (int o = 128; o > 0; o >>= 1) { if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o]; __syncthreads(); }
        c2 = red[0]; __syncthreads();
    }
    for (int i = threadIdx.x; i < p.nblk1; i += 256) a += (double)p.part1[i];
    for (int i = threadIdx.x; i < p.nblk2; i += 256) b += (double)p.part2[i];
    red[threadIdx.x] = a; __syncthreads();
    for (int o = 128; o > 0; o >>= 1) { if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o]; __syncthreads(); }
    const double l1 = red[0]; __syncthreads();
    red[threadIdx.x] = b; __syncthreads();
    for (int o = 128; o > 0; o >>= 1) { if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o]; __syncthreads(); }
    if (threadIdx.x == 0) {
        const double n1 = MASKED ? c1 * 3.0 : (double)p.B * p.H * p.W * 3.0;
        const double n2 = MASKED ? c2 * 3.0 : (double)p.B * (p.H - 2) * (p.W - 2) * 3.0;
        const double ms = (MASKED && c2 == 0.0) ? 0.0 : red[0] / n2, ml = (MASKED && c1 == 0.0) ? 0.0 : l1 / n1;
        p.result[0] = (float)(0.85 * ms + 0.15 * ml);
        p.result[1] = (float)ms;
        p.result[2] = (float)ml;
    }
}

// ------------------------------------------------------------------------------------------
// edge-aware smoothness (Losses/loss_factory.py:183-220): S = mean(|Kx * x| exp(-|Kx * y|) + |Ky * x| exp(-|Ky * y|)), x = disp / 255, y = image / 255
// ------------------------------------------------------------------------------------------
struct SmoothArgs {
    const float* disp; const float* image; float* part; float* result; float* ddisp;
    int B, H, W, C, nblk, accumulate;
    float weight, grad_scale;
};

// One launch for the value and the gradient, tiled like loss_tile_kernel (LT_H x LT_W pixels per workgroup, all through LDS):
//   A  x / 255 and the channel sum of y / 255 at the tile + a 2-pixel halo (outside the image: the zeros of SAME padding, also across the batch);
//   B  both stencils of both maps at the tile + a 1-pixel halo -> s_x = sign(gx) exp(-|ix|), s_y likewise (outside the image: zero -- no term lives there);
//      partial sum of |gx| exp(-|ix|) + |gy| exp(-|iy|) over the tile's own pixels;
//   C  d S / d x[p] = the transposed stencils gathered at p: sum_ij Kx[i][j] s_x(p - (i-1, j-1)) + Ky[i][j] s_y(p - (i-1, j-1)); one thread per element.
// The reference's sobel_y literal has -1 top right (:198); kept.
#define SM_HH (LT_H + 4)
#define SM_HW (LT_W + 4)
#define SM_WH (LT_H + 2)
#define SM_WW (LT_W + 2)
// s: top-left of a 3x3 window in an array of row stride LD -> Kx * s, Ky * s at its centre
template <int LD> __device__ __forceinline__ void smooth_stencils(const float* s, float& gx, float& gy) {
    const float a00 = s[0], a01 = s[1], a02 = s[2], a10 = s[LD], a12 = s[LD + 2], a20 = s[2 * LD], a21 = s[2 * LD + 1], a22 = s[2 * LD + 2];
    gx = (a00 - a02) + 2.f * (a10 - a12) + (a20 - a22);
    gy = (a00 + 2.f * a01 - a02) - (a20 + 2.f * a21 + a22);
}
__global__ __launch_bounds__(256) void smooth_tile_kernel(SmoothArgs p, int tiles_x, int tiles_y) {
    __shared__ float red[4];
    __shared__ float s_d[SM_HH * SM_HW];
    __shared__ float s_i[SM_HH * SM_HW];
    __shared__ float s_sx[SM_WH * SM_WW];
    __shared__ float s_sy[SM_WH * SM_WW];
    const int tid = threadIdx.x;
    const int tx = blockIdx.x % tiles_x;
    const int t2 = blockIdx.x / tiles_x;
    const int ty = t2 % tiles_y, b = t2 / tiles_y;
    const int y0t = ty * LT_H, x0t = tx * LT_W;
    // ---- A -------------------------------------------------------------------------------------
    for (int i = tid; i < SM_HH * SM_HW; i += 256) {
        const int ly = i / SM_HW, lx = i - ly * SM_HW;
        const int y = y0t - 2 + ly, x = x0t - 2 + lx;
        float dv = 0.f, iv = 0.f;
        if ((unsigned)y < (unsigned)p.H && (unsigned)x < (unsigned)p.W) {
            const int64_t q = ((int64_t)b * p.H + y) * p.W + x;
            dv = p.disp[q] / 255.0f;
            if (p.C == 3) {
                const float* im = p.image + q * 3;
                iv = im[0] / 255.0f + im[1] / 255.0f + im[2] / 255.0f;
            } else {
                iv = p.image[q] / 255.0f;
            }
        }
        s_d[i] = dv; s_i[i] = iv;
    }
    __syncthreads();
    // ---- B -------------------------------------------------------------------------------------
    float term = 0.f;
    for (int i = tid; i < SM_WH * SM_WW; i += 256) {
        const int ly = i / SM_WW, lx = i - ly * SM_WW;
        const int y = y0t - 1 + ly, x = x0t - 1 + lx;
        float sx = 0.f, sy = 0.f;
        if ((unsigned)y < (unsigned)p.H && (unsigned)x < (unsigned)p.W) {
            float gx, gy, ix, iy;
            smooth_stencils<SM_HW>(s_d + ly * SM_HW + lx, gx, gy);
            smooth_stencils<SM_HW>(s_i + ly * SM_HW + lx, ix, iy);
            const float wx = expf(-fabsf(ix)), wy = expf(-fabsf(iy));      // the accurate exp: |ix| reaches 24 on 8-bit frames
            sx = gx > 0.f ? wx : (gx < 0.f ? -wx : 0.f);
            sy = gy > 0.f ? wy : (gy < 0.f ? -wy : 0.f);
            if (ly >= 1 && lx >= 1 && ly <= LT_H && lx <= LT_W) term += fabsf(gx) * wx + fabsf(gy) * wy;
        }
        s_sx[i] = sx; s_sy[i] = sy;
    }
    const float tot = block_sum(term, red);          // (its barriers also publish s_sx / s_sy)
    if (tid == 0) p.part[blockIdx.x] = tot;
    if (!p.ddisp) return;
    // ---- C -------------------------------------------------------------------------------------
    const float k = p.grad_scale * p.weight / (255.0f * ((float)p.B * (float)p.H * (float)p.W));
    for (int i = tid; i < LT_H * LT_W; i += 256) {
        const int iy = i / LT_W, ix = i - iy * LT_W;
        const int y = y0t + iy, x = x0t + ix;
        if (y >= p.H || x >= p.W) continue;
        // s(p - (i-1, j-1)) for i, j = 0 .. 2 = local (iy + 2 - i, ix + 2 - j): the window read back to front
        const float* ax = s_sx + iy * SM_WW + ix;
        const float* ay = s_sy + iy * SM_WW + ix;
        const float g = (ax[2 * SM_WW + 2] - ax[2 * SM_WW]) + 2.f * (ax[SM_WW + 2] - ax[SM_WW]) + (ax[2] - ax[0])
                      + (ay[2 * SM_WW + 2] + 2.f * ay[2 * SM_WW + 1] - ay[2 * SM_WW]) - (ay[2] + 2.f * ay[1] + ay[0]);
        const int64_t q = ((int64_t)b * p.H + y) * p.W + x;
        p.ddisp[q] = p.accumulate ? p.ddisp[q] + k * g : k * g;
    }
}

__global__ __launch_bounds__(256) void smooth_final_kernel(SmoothArgs p) {
    __shared__ double red[256];
    double a = 0.0;
    for (int i = threadIdx.x; i < p.nblk; i += 256) a += (double)p.part[i];
    red[threadIdx.x] = a; __syncthreads();
    for (int o = 128; o > 0; o >>= 1) { if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o]; __syncthreads(); }
    if (threadIdx.x == 0) {
        const float v = (float)((double)p.weight * (red[0] / ((double)p.B * p.H * p.W)));
        p.result[3] = v;
        p.result[0] = p.accumulate ? p.result[0] + v : v;
    }
}

// ------------------------------------------------------------------------------------------
// validation metrics (Stereo_Online_Adaptation.py:74-82)
// ------------------------------------------------------------------------------------------
struct MetArgs { const float* disp; const float* gt; float* part; float* result; int64_t total; int nblk; float th; };

__global__ __launch_bounds__(256) void metrics_kernel(MetArgs p) {
    __shared__ float red[4];
    const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
    float e = 0.f, bad = 0.f, v = 0.f;
    if (q < p.total) {
        const float gt = p.gt[q];
        v = (gt == 0.f) ? 0.f : 1.f;
        e = fabsf(p.disp[q] - gt) * v;
        bad = e > p.th ? 1.f : 0.f;
    }
    const float se = block_sum(e, red);
    const float sb = block_sum(bad, red);
    const float sv = block_sum(v, red);
    if (threadIdx.x == 0) { p.part[blockIdx.x * 3 + 0] = se; p.part[blockIdx.x * 3 + 1] = sb; p.part[blockIdx.x * 3 + 2] = sv; }
}

__global__ __launch_bounds__(256) void metrics_final_kernel(MetArgs p) {
    __shared__ double red[3][256];
    double a = 0, b = 0, c = 0;
    for (int i = threadIdx.x; i < p.nblk; i += 256) { a += p.part[i * 3]; b += p.part[i * 3 + 1]; c += p.part[i * 3 + 2]; }
    red[0][threadIdx.x] = a; red[1][threadIdx.x] = b; red[2][threadIdx.x] = c;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) {
            red[0][threadIdx.x] += red[0][threadIdx.x + o];
            red[1][threadIdx.x] += red[1][threadIdx.x + o];
            red[2][threadIdx.x] += red[2][threadIdx.x + o];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        p.result[0] = (float)(red[0][0] / red[2][0]);
        p.result[1] = (float)(red[1][0] / red[2][0]);
        p.result[2] = (float)red[2][0];
    }
}

// ------------------------------------------------------------------------------------------
// proxy-label loss of the continual-adaptation variant: loss_factory.get_proxy_loss('mean_l1') (Losses/loss_factory.py:304-351)
//   valid = !(proxy <= 0 || proxy >= 192) ; loss = weight * sum(valid * |pred - proxy|) / sum(valid)
//   d loss / d pred = weight * valid * sign(pred - proxy) / sum(valid)       (tf.abs gradient: sign, 0 at 0)
// ------------------------------------------------------------------------------------------
// The supervised multi-scale loss of Train.py (loss_factory.get_supervised_loss('mean_l1'), Losses/loss_factory.py:256-302) is the
// same reduction with valid = !(target == 0 || target >= max_disp): `hi` / `zero_only` select the rule.
//
// mh_label_loss: the same reduction for the six scalar (x, y, mask) losses of the reference's table (Losses/loss_factory.py:28-108), FAM = the per-pixel term
//   0  l1     phi = |d|                                  phi' = sign(d), 0 at 0
//   1  l2     phi = d^2                                  phi' = 2 d
//   2  huber  phi = d > 1 ? 0.5 + (|d| - 1) : 0.5 d^2    phi' = d > 1 ? 1 : d       (:52-58: the test is on the SIGNED d -- a large negative error stays
//                                                                                    quadratic -- and d == 1 is quadratic)
// and `norm` = the normaliser where it does not depend on the data (sum_*: 1; mean_huber: the number of pixels, valid or not -- tf.reduce_mean(huber * mask), :71),
// 0 = sum(valid) (mean_l1, mean_l2).  With a fixed normaliser the partial kernel writes the gradient too (FUSED) and the op is two launches.  The kernels are
// templated on FAM: FAM 0 with norm 0 is the code mh_proxy_loss / mh_supervised_loss always ran, so MH_LOSS_MEAN_L1 has their bits.
struct ProxyArgs { const float* pred; const float* proxy; float* part; float* result; float* dpred; int64_t total; int nblk; float weight, gs; float hi; int zero_only;
                   float norm; };
__device__ __forceinline__ float proxy_valid(const ProxyArgs& p, float px) {
    const bool bad = (p.zero_only ? px == 0.f : px <= 0.f) || px >= p.hi;
    return bad ? 0.f : 1.f;
}

template <int FAM> __device__ __forceinline__ float label_phi(float d) {
    if (FAM == 0) return fabsf(d);
    if (FAM == 1) return d * d;
    return d > 1.0f ? 0.5f + (fabsf(d) - 1.0f) : 0.5f * (d * d);
}

template <int FAM> __device__ __forceinline__ float label_dphi(float d) {
    if (FAM == 0) return d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f);
    if (FAM == 1) return 2.0f * d;
    return d > 1.0f ? 1.0f : d;
}

template <int FAM, bool FUSED> __global__ __launch_bounds__(256) void proxy_partial_kernel(ProxyArgs p) {
    __shared__ float red[4];
    const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
    float e = 0.f, v = 0.f;
    if (q < p.total) {
        const float px = p.proxy[q];
        v = proxy_valid(p, px);
        const float d = p.pred[q] - px;
        e = label_phi<FAM>(d) * v;
        if (FUSED) p.dpred[q] = p.gs * p.weight * v * label_dphi<FAM>(d) / p.norm;
    }
    const float se = block_sum(e, red);
    const float sv = block_sum(v, red);
    if (threadIdx.x == 0) { p.part[blockIdx.x * 2 + 0] = se; p.part[blockIdx.x * 2 + 1] = sv; }
}

// (norm > 0: the fixed normaliser instead of sum(valid))
__global__ __launch_bounds__(256) void proxy_final_kernel(ProxyArgs p) {
    __shared__ double red[2][256];
    double a = 0, c = 0;
    for (int i = threadIdx.x; i < p.nblk; i += 256) { a += p.part[i * 2]; c += p.part[i * 2 + 1]; }
    red[0][threadIdx.x] = a; red[1][threadIdx.x] = c;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) { red[0][threadIdx.x] += red[0][threadIdx.x + o]; red[1][threadIdx.x] += red[1][threadIdx.x + o]; }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const double n = p.norm > 0.f ? (double)p.norm : red[1][0];
        p.result[0] = (float)((double)p.weight * red[0][0] / n);              // 0/0 = NaN like the TF graph
        p.result[1] = (float)red[1][0];
    }
}

template <int FAM> __global__ __launch_bounds__(256) void proxy_grad_kernel(ProxyArgs p) {
    const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (q >= p.total) return;
    const float px = p.proxy[q];
    const float v = proxy_valid(p, px);
    const float d = p.pred[q] - px;
    p.dpred[q] = p.gs * p.weight * v * label_dphi<FAM>(d) / p.result[1];
}

// ------------------------------------------------------------------------------------------
// the MAD blocks' proxy loss at 1/s scale (Stereo_Continual_Adaptation.py:26-27,95-112 with --reprojectionScale s): the block's
// full-size prediction and the proxy labels are both resized (TF1 legacy bilinear, interp1 / bilerp above) to Hs x Ws = H//s x W//s, the
// proxy divided by s:   p = R(pred),  q = R(proxy) / s,  valid = !(q <= 0 || q >= 192),  loss = weight * sum(valid |p - q|) / sum(valid),
//   d loss / d pred = grad_scale * weight * R^T(valid * sign(p - q)) / sum(valid)        on the full H x W grid.
// Both maps are sampled on the fly -- launch 1 for the partial sums, launch 3 again per candidate output pixel of a source pixel (the gather
// walk of resize_bwd_kernel, fixed order, no atomics, every element of dpred written); launch 2 is proxy_final_kernel.
// ------------------------------------------------------------------------------------------
// mh_label_loss_scaled: FAM / norm as for ProxyArgs above (mean_huber: norm = B * Hs * Ws).  With a fixed normaliser ONE launch does both walks
// (proxy_s_fused_kernel: the partial sums by its first workgroups, the gather walk by all of them), so the op is two launches.
struct ProxySArgs { const float* pred; const float* proxy; float* part; const float* result; float* dpred; int B, H, W, Hs, Ws; float sy, sx, fs, weight, gs;
                    float norm; };

// interp1 without mul+sub contraction: t is EXACTLY fl(i * scale) - lo.  Where fl(i * scale) is an integer (row 21 of 128 -> 42 rows: 21 * fl(128 / 42) rounds to 64) the
// upper tap must carry the weight 0, not the 5e-7 an fma leaves behind: a label whose lower taps are holes (exactly 0) is then exactly 0 -- invalid -- in both launches
// and in any other arithmetic that rounds the product first, instead of a tiny valid value in whichever launch the compiler happened to contract.
__device__ __forceinline__ void interp1_exact(int i, float scale, int n, int& lo, int& hi, float& t) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const float src = (float)i * scale;
    lo = (int)src;
    hi = min(lo + 1, n - 1);
    t = src - (float)lo;
}

// p - q at one output pixel whose taps are given; v = its validity
__device__ __forceinline__ float proxy_s_diff(const ProxySArgs& p, const float* pred, const float* proxy, int y0, int y1, float ty, int x0, int x1, float tx,
                                              float& v) {
    const float pv = bilerp(pred, p.W, y0, y1, ty, x0, x1, tx, 1.0f, false);
    const float q = bilerp(proxy, p.W, y0, y1, ty, x0, x1, tx, 1.0f, false) / p.fs;
    v = (q <= 0.f || q >= 192.0f) ? 0.f : 1.f;
    return pv - q;
}

template <int FAM> __device__ __forceinline__ void proxy_s_partial(const ProxySArgs& p, float* red) {
    const int64_t total = (int64_t)p.B * p.Hs * p.Ws;
    const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
    float e = 0.f, v = 0.f;
    if (q < total) {
        const int x = (int)(q % p.Ws);
        const int64_t t2 = q / p.Ws;
        const int y = (int)(t2 % p.Hs);
        const int64_t off = (t2 / p.Hs) * p.H * p.W;
        int y0, y1, x0, x1; float ty, tx;
        interp1_exact(y, p.sy, p.H, y0, y1, ty);
        interp1_exact(x, p.sx, p.W, x0, x1, tx);
        e = label_phi<FAM>(proxy_s_diff(p, p.pred + off, p.proxy + off, y0, y1, ty, x0, x1, tx, v)) * v;
    }
    const float se = block_sum(e, red);
    const float sv = block_sum(v, red);
    if (threadIdx.x == 0) { p.part[blockIdx.x * 2 + 0] = se; p.part[blockIdx.x * 2 + 1] = sv; }
}

// one lane per SOURCE pixel: the output pixels whose lower / upper tap is this pixel, rows outside, columns inside (resize_bwd_kernel's candidate window)
template <int FAM> __device__ __forceinline__ void proxy_s_grad(const ProxySArgs& p, float nvalid) {
    const int64_t total = (int64_t)p.B * p.H * p.W;
    const float isy = 1.0f / p.sy, isx = 1.0f / p.sx;
    const float k = p.gs * p.weight;
    for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < total; q += (int64_t)gridDim.x * 256) {
        const int sx = (int)(q % p.W);
        const int64_t t2 = q / p.W;
        const int sy = (int)(t2 % p.H);
        const int64_t off = (t2 / p.H) * p.H * p.W;
        const int ya = max(0, (int)floorf((float)(sy - 1) * isy) - 1), yb = min(p.Hs - 1, (int)ceilf((float)(sy + 1) * isy) + 1);
        const int xa = max(0, (int)floorf((float)(sx - 1) * isx) - 1), xb = min(p.Ws - 1, (int)ceilf((float)(sx + 1) * isx) + 1);
        float acc = 0.f;
        for (int Y = ya; Y <= yb; ++Y) {
            int y0, y1; float ty;
            interp1_exact(Y, p.sy, p.H, y0, y1, ty);
            const float wy = (y0 == sy ? 1.0f - ty : 0.f) + (y1 == sy ? ty : 0.f);
            if (wy == 0.f) continue;
            for (int X = xa; X <= xb; ++X) {
                int x0, x1; float tx;
                interp1_exact(X, p.sx, p.W, x0, x1, tx);
                const float wx = (x0 == sx ? 1.0f - tx : 0.f) + (x1 == sx ? tx : 0.f);
                if (wx == 0.f) continue;
                float v;
                const float d = proxy_s_diff(p, p.pred + off, p.proxy + off, y0, y1, ty, x0, x1, tx, v);
                const float sgn = label_dphi<FAM>(d);
                acc += v * sgn * wy * wx;
            }
        }
        p.dpred[q] = k * acc / nvalid;
    }
}

template <int FAM> __global__ __launch_bounds__(256) void proxy_s_partial_kernel(ProxySArgs p) {
    __shared__ float red[4];
    proxy_s_partial<FAM>(p, red);
}

template <int FAM> __global__ __launch_bounds__(256) void proxy_s_grad_kernel(ProxySArgs p) { proxy_s_grad<FAM>(p, p.result[1]); }

// fixed normaliser: workgroups 0 .. nblk - 1 first take their 256 output pixels' partial sums, then every workgroup joins the gather walk
template <int FAM> __global__ __launch_bounds__(256) void proxy_s_fused_kernel(ProxySArgs p, int nblk) {
    __shared__ float red[4];
    if ((int)blockIdx.x < nblk) proxy_s_partial<FAM>(p, red);
    proxy_s_grad<FAM>(p, p.norm);
}

// ------------------------------------------------------------------------------------------
// KITTI D1-all and EPE of the continual loop (Stereo_Continual_Adaptation.py:245-249): val = gt > 0, diff = |gt - disp| on val,
// outlier = diff > 3 && diff / gt >= 0.05.  The error sum of a workgroup is taken in double (the report prints three decimals of a mean
// over ~4e5 pixels); counts are exact in float.
// ------------------------------------------------------------------------------------------
struct KittiArgs { const float* disp; const float* gt; float* part; float* result; int64_t total; int nblk; };

__global__ __launch_bounds__(256) void metrics_kitti_kernel(KittiArgs p) {
    __shared__ float red[4];
    __shared__ double dred[256];
    const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
    float diff = 0.f, bad = 0.f, v = 0.f;
    if (q < p.total) {
        const float gt = p.gt[q];
        if (gt > 0.f) {
            v = 1.f;
            diff = fabsf(gt - p.disp[q]);
            bad = (diff > 3.0f && diff / gt >= 0.05f) ? 1.f : 0.f;
        }
    }
    dred[threadIdx.x] = (double)diff;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) { if ((int)threadIdx.x < o) dred[threadIdx.x] += dred[threadIdx.x + o]; __syncthreads(); }
    const float sb = block_sum(bad, red);
    const float sv = block_sum(v, red);
    if (threadIdx.x == 0) { p.part[blockIdx.x * 3 + 0] = (float)dred[0]; p.part[blockIdx.x * 3 + 1] = sb; p.part[blockIdx.x * 3 + 2] = sv; }
}

__global__ __launch_bounds__(256) void metrics_kitti_final_kernel(KittiArgs p) {
    __shared__ double red[3][256];
    double a = 0, b = 0, c = 0;
    for (int i = threadIdx.x; i < p.nblk; i += 256) { a += p.part[i * 3]; b += p.part[i * 3 + 1]; c += p.part[i * 3 + 2]; }
    red[0][threadIdx.x] = a; red[1][threadIdx.x] = b; red[2][threadIdx.x] = c;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) {
            red[0][threadIdx.x] += red[0][threadIdx.x + o];
            red[1][threadIdx.x] += red[1][threadIdx.x + o];
            red[2][threadIdx.x] += red[2][threadIdx.x + o];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        p.result[0] = (float)(red[0][0] / red[2][0]);               // no valid pixel: 0/0 = NaN, like np.mean of an empty selection
        p.result[1] = (float)(100.0 * (red[1][0] / red[2][0]));
        p.result[2] = (float)red[2][0];
    }
}

// ------------------------------------------------------------------------------------------
// momentum / glue
// ------------------------------------------------------------------------------------------
// 16-byte form (all three buffers 16-byte aligned: the engines' flat buffers are): two loads in flight per lane, the launch sits behind the join
// at the very end of the step.  Same arithmetic per element.
__global__ __launch_bounds__(256) void momentum4_kernel(float4* var, float4* acc, const float4* g, int64_t n4, float lr, float mom, float gs) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
        const float4 m = acc[i], gg = g[i];
        float4 v = var[i];
        float4 a;
        a.x = mom * m.x + gs * gg.x; a.y = mom * m.y + gs * gg.y; a.z = mom * m.z + gs * gg.z; a.w = mom * m.w + gs * gg.w;
        acc[i] = a;
        v.x -= lr * a.x; v.y -= lr * a.y; v.z -= lr * a.z; v.w -= lr * a.w;
        var[i] = v;
    }
}
__global__ __launch_bounds__(256) void momentum_kernel(float* var, float* acc, const float* g, int64_t n, float lr, float mom, float gs) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const float a = mom * acc[i] + gs * g[i];
        acc[i] = a;
        var[i] -= lr * a;
    }
}

// tf.train.AdamOptimizer(lr, beta1) of Train.py:95 (TF 1.12 training/adam.py, ApplyAdam):
//   lr_t = lr * sqrt(1 - beta2_power) / (1 - beta1_power);  m += (g - m)(1 - b1);  v += (g^2 - v)(1 - b2);
//   var -= (m * lr_t) / (sqrt(v) + eps)         state = {beta1_power, beta2_power}, multiplied by b1 / b2 AFTER the update
__global__ __launch_bounds__(256) void adam_kernel(float* var, float* m, float* v, const float* g, int64_t n, const float* state,
                                                   float lr, float b1, float b2, float eps, float gs) {
    const float lr_t = lr * sqrtf(1.0f - state[1]) / (1.0f - state[0]);
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const float gi = gs * g[i];
        const float mi = m[i] + (gi - m[i]) * (1.0f - b1);          // the ApplyAdam functor's own form (core/kernels/training_ops.cc)
        const float vi = v[i] + (gi * gi - v[i]) * (1.0f - b2);
        m[i] = mi; v[i] = vi;
        var[i] -= (mi * lr_t) / (sqrtf(vi) + eps);
    }
}
__global__ void adam_advance_kernel(float* state, float b1, float b2) {
    if (threadIdx.x == 0 && blockIdx.x == 0) { state[0] *= b1; state[1] *= b2; }
}

__global__ __launch_bounds__(256) void copy_channels_kernel(const float* src, int src_ld, float* dst, int dst_ld, int64_t npix,
                                                            int nch, float scale, int accumulate) {
    const int64_t total = npix * nch;
    for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < total; q += (int64_t)gridDim.x * 256) {
        const int c = (int)(q % nch);
        const int64_t pix = q / nch;
        const float v = scale * src[pix * src_ld + c];
        float* d = dst + pix * dst_ld + c;
        *d = accumulate ? *d + v : v;
    }
}

__global__ __launch_bounds__(256) void leaky_bwd_kernel(float* dy, int dy_ld, const float* y, int y_ld, int64_t npix, int nch, float alpha) {
    const int64_t total = npix * nch;
    for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < total; q += (int64_t)gridDim.x * 256) {
        const int c = (int)(q % nch);
        const int64_t pix = q / nch;
        if (!(y[pix * y_ld + c] > 0.f)) dy[pix * dy_ld + c] *= alpha;
    }
}

// column sums, coalesced along the channels: a wave row = 64/nchp pixels x nchp channels (nchp = power of two covering
// min(nch, 64)), blockIdx.y = 64-channel chunk; pixels strided over waves and workgroups; shuffle reduction over the
// pixels of a wave row, LDS over the 4 waves, one atomic per channel per workgroup.
__global__ __launch_bounds__(256) void bias_grad_kernel(const float* dz, int dz_ld, int64_t npix, int nch, float* db, int nchp, float* ws) {
    __shared__ float red[4][64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int ppw = 64 / nchp;
    const int c = blockIdx.y * 64 + (lane & (nchp - 1));
    const int pl = lane / nchp;
    float v = 0.f;
    if (c < nch) {
        // eight loads in flight per lane (one per iteration left the launch latency bound: 15 - 30 dependent round trips on DispNet's 192x640 maps)
        const int64_t st = (int64_t)gridDim.x * 4 * ppw;
        int64_t q = ((int64_t)blockIdx.x * 4 + w) * ppw + pl;
        float a[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        for (; q + 7 * st < npix; q += 8 * st) {
            float t[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) t[u] = dz[(q + u * st) * dz_ld + c];
#pragma unroll
            for (int u = 0; u < 8; ++u) a[u] += t[u];
        }
        for (; q < npix; q += st) a[0] += dz[q * dz_ld + c];
        v = ((a[0] + a[1]) + (a[2] + a[3])) + ((a[4] + a[5]) + (a[6] + a[7]));
    }
    for (int o = nchp; o < 64; o <<= 1) v += __shfl_xor(v, o);
    red[w][lane] = v;
    __syncthreads();
    if (w == 0 && pl == 0 && c < nch) {
        const float t = (red[0][lane] + red[1][lane]) + (red[2][lane] + red[3][lane]);
        // partial form (round 6): the workgroup's column sums go to ws[blockIdx.x][nch] with plain stores and mh_wgrad_reduce sums the workgroups in order
        if (ws) ws[(int64_t)blockIdx.x * nch + c] = t; else mh_atomic_add(db + c, t);
    }
}

__global__ __launch_bounds__(256) void fill_kernel(float* p, int64_t n, float v) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) p[i] = v;
}

inline int grid_for(int64_t n, int cap = 256 * 16) {
    int64_t b = (n + 255) / 256;
    if (b > cap) b = cap;
    if (b < 1) b = 1;
    return (int)b;
}

}  // namespace

extern "C" int mh_warp_fwd(const float* img, int32_t img_ld, const float* u, float* out, int32_t out_ld,
                           int32_t B, int32_t H, int32_t W, int32_t C, void* stream) {
    MH_REQUIRE(img && u && out, MH_ERR_ARG, "mh_warp_fwd: null argument");
    MH_REQUIRE(B > 0 && H > 0 && W > 0 && C > 0, MH_ERR_ARG, "mh_warp_fwd: bad dimension");
    MH_REQUIRE(C % 4 == 0 && img_ld % 4 == 0 && out_ld % 4 == 0 && mh_aligned16(img) && mh_aligned16(out), MH_ERR_ALIGN,
               "mh_warp_fwd: C and lds must be multiples of 4, pointers 16-byte aligned");
    WarpArgs a{}; a.img = img; a.u = u; a.out = out; a.img_ld = img_ld; a.out_ld = out_ld;
    a.B = B; a.H = H; a.W = W; a.C = C; a.total = (int64_t)B * H * W * (C / 4);
    hipLaunchKernelGGL(warp_fwd_kernel, dim3(grid_for(a.total)), dim3(256), 0, (hipStream_t)stream, a);
    return mh_check_launch("warp_fwd");
}

extern "C" int mh_warp_bwd(const float* g, int32_t g_ld, const float* img, int32_t img_ld, const float* u,
                           float* dimg, int32_t dimg_ld, float* du, int32_t acc_u,
                           int32_t B, int32_t H, int32_t W, int32_t C, void* stream) {
    MH_REQUIRE(g && img && u && (dimg || du), MH_ERR_ARG, "mh_warp_bwd: null argument");
    MH_REQUIRE(B > 0 && H > 0 && W > 0 && C > 0, MH_ERR_ARG, "mh_warp_bwd: bad dimension");
    MH_REQUIRE(C % 4 == 0 && img_ld % 4 == 0 && g_ld % 4 == 0 && mh_aligned16(img) && mh_aligned16(g), MH_ERR_ALIGN,
               "mh_warp_bwd: C and lds must be multiples of 4, pointers 16-byte aligned");
    WarpArgs a{}; a.g = g; a.img = img; a.u = u; a.dimg = dimg; a.du = du; a.acc_u = acc_u;
    a.g_ld = g_ld; a.img_ld = img_ld; a.dimg_ld = dimg_ld; a.B = B; a.H = H; a.W = W; a.C = C;
    const int C4 = C / 4;
    const int64_t npix = (int64_t)B * H * W;
    hipStream_t s = (hipStream_t)stream;
    if (C4 <= 4) hipLaunchKernelGGL((warp_bwd_kernel<4>), dim3(grid_for(npix * 4)), dim3(256), 0, s, a);
    else if (C4 <= 8) hipLaunchKernelGGL((warp_bwd_kernel<8>), dim3(grid_for(npix * 8)), dim3(256), 0, s, a);
    else hipLaunchKernelGGL((warp_bwd_kernel<16>), dim3(grid_for(npix * 16)), dim3(256), 0, s, a);
    return mh_check_launch("warp_bwd");
}

static int resize_args(ResizeArgs& a, int B, int Hi, int Wi, int Hr, int Wr, int cy, int cx, int Ho, int Wo, float mul, int mode) {
    MH_REQUIRE(B > 0 && Hi > 0 && Wi > 0 && Hr > 0 && Wr > 0 && Ho > 0 && Wo > 0, MH_ERR_ARG, "mh_resize: bad dimension");
    MH_REQUIRE(cy >= 0 && cx >= 0 && cy + Ho <= Hr && cx + Wo <= Wr, MH_ERR_ARG, "mh_resize: crop outside the resized image");
    MH_REQUIRE(mode >= 0 && mode <= 2, MH_ERR_ARG, "mh_resize: mode must be 0,1,2");
    a.B = B; a.Hi = Hi; a.Wi = Wi; a.Hr = Hr; a.Wr = Wr; a.cy = cy; a.cx = cx; a.Ho = Ho; a.Wo = Wo; a.mode = mode;
    a.mul = mul; a.sy = (float)Hi / (float)Hr; a.sx = (float)Wi / (float)Wr;
    return 0;
}

extern "C" int mh_resize_fwd(const float* in, float* out, int32_t B, int32_t Hi, int32_t Wi, int32_t Hr, int32_t Wr,
                             int32_t cy, int32_t cx, int32_t Ho, int32_t Wo, float mul, int32_t mode, void* stream) {
    MH_REQUIRE(in && out, MH_ERR_ARG, "mh_resize_fwd: null argument");
    ResizeArgs a{}; a.in = in; a.out = out;
    if (int e = resize_args(a, B, Hi, Wi, Hr, Wr, cy, cx, Ho, Wo, mul, mode)) return e;
    hipLaunchKernelGGL(resize_fwd_kernel, dim3(grid_for((int64_t)B * Ho * Wo)), dim3(256), 0, (hipStream_t)stream, a);
    return mh_check_launch("resize_fwd");
}

// uint8 frames (what the camera / the PNG decoder delivers) -> float32 0..255 (what the graph reads): the cast tf.data does on the
// host (Data_utils/data_reader.py:98 tf.cast(..., tf.float32)) moved behind the PCIe copy, which then carries 1 byte per value
__global__ __launch_bounds__(256) void u8_to_f32_kernel(const unsigned char* __restrict__ in, float* __restrict__ out, int64_t n) {
    const int64_t q4 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4;
    if (q4 + 4 <= n && ((((uintptr_t)in) | ((uintptr_t)out)) & 3u) == 0 && (((uintptr_t)out) & 15u) == 0) {
        const unsigned v = *reinterpret_cast<const unsigned*>(in + q4);
        *reinterpret_cast<float4*>(out + q4) = make_float4((float)(v & 0xffu), (float)((v >> 8) & 0xffu), (float)((v >> 16) & 0xffu), (float)(v >> 24));
    } else {
        for (int64_t q = q4; q < q4 + 4 && q < n; ++q) out[q] = (float)in[q];
    }
}

// ---- the step's frames through a table the HOST rewrites between two replays of a captured step (mh_fetch_inputs) ---------------------------------------------------
// A captured step reads its frames at fixed addresses; a prefetcher delivers frame t in slot t % depth.  Instead of three copy launches in front of every replay, the
// step's first node reads the slot's addresses from a small table (device-visible host memory, or device memory the host updates) and moves / casts the frames into the
// fixed input buffers itself.  Entry k: src[k] = NULL or == dst[k]: nothing to do; u8[k]: the source holds 8-bit values.
struct FetchArgs { const mh_input_table* tab; float* dst[MH_FETCH_MAX]; int64_t n[MH_FETCH_MAX]; int64_t q0[MH_FETCH_MAX + 1]; };
__global__ __launch_bounds__(256) void fetch_inputs_kernel(FetchArgs a) {
    const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;          // one quad of floats
    int k = 0;
#pragma unroll
    for (int j = 1; j < MH_FETCH_MAX; ++j) k += q >= a.q0[j] ? 1 : 0;
    if (q >= a.q0[MH_FETCH_MAX]) return;
    const void* src = a.tab->src[k];
    float* dst = a.dst[k];
    if (!src || src == (const void*)dst) return;
    const int64_t e0 = (q - a.q0[k]) * 4, n = a.n[k];
    if (a.tab->u8[k]) {
        const unsigned char* in = (const unsigned char*)src;
        if (e0 + 4 <= n && ((((uintptr_t)in) & 3u) | (((uintptr_t)dst) & 15u)) == 0) {
            const unsigned v = *reinterpret_cast<const unsigned*>(in + e0);
            *reinterpret_cast<float4*>(dst + e0) = make_float4((float)(v & 0xffu), (float)((v >> 8) & 0xffu), (float)((v >> 16) & 0xffu), (float)(v >> 24));
        } else {
            for (int64_t e = e0; e < e0 + 4 && e < n; ++e) dst[e] = (float)in[e];
        }
    } else {
        const float* in = (const float*)src;
        if (e0 + 4 <= n && ((((uintptr_t)in) | ((uintptr_t)dst)) & 15u) == 0) *reinterpret_cast<float4*>(dst + e0) = *reinterpret_cast<const float4*>(in + e0);
        else for (int64_t e = e0; e < e0 + 4 && e < n; ++e) dst[e] = in[e];
    }
}

extern "C" int mh_fetch_inputs(const mh_input_table* table, float* const* dst, const int64_t* n, int32_t count, void* stream) {
    MH_REQUIRE(table && dst && n && count >= 1 && count <= MH_FETCH_MAX, MH_ERR_ARG, "mh_fetch_inputs: bad argument");
    FetchArgs a{};
    a.tab = table;
    int64_t q = 0;
    for (int k = 0; k < MH_FETCH_MAX; ++k) {
        a.q0[k] = q;
        if (k < count) {
            MH_REQUIRE(dst[k] && n[k] >= 0, MH_ERR_ARG, "mh_fetch_inputs: null destination / negative count");
            a.dst[k] = dst[k]; a.n[k] = n[k];
            q += (n[k] + 3) / 4;
        }
    }
    a.q0[MH_FETCH_MAX] = q;
    if (q == 0) return 0;
    MH_REQUIRE((q + 255) / 256 < (1ll << 31), MH_ERR_UNSUPPORTED, "mh_fetch_inputs: too many elements");
    hipLaunchKernelGGL(fetch_inputs_kernel, dim3((unsigned)((q + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a);
    return mh_check_launch("fetch_inputs");
}

// the device-side address of a page-locked host allocation (what a kernel dereferences to read a table the host keeps writing)
extern "C" int mh_host_device_pointer(void* host, void** device) {
    MH_REQUIRE(host && device, MH_ERR_ARG, "mh_host_device_pointer: null argument");
    hipError_t e = hipHostGetDevicePointer(device, host, 0);
    if (e != hipSuccess) { mh_set_error("mh_host_device_pointer: %s", hipGetErrorString(e)); return (int)e; }
    return 0;
}

extern "C" int mh_u8_to_f32(const uint8_t* in, float* out, int64_t n, void* stream) {
    MH_REQUIRE(in && out && n > 0, MH_ERR_ARG, "mh_u8_to_f32: bad argument");
    MH_REQUIRE((n + 1023) / 1024 < (1ll << 31), MH_ERR_UNSUPPORTED, "mh_u8_to_f32: too many elements");
    hipLaunchKernelGGL(u8_to_f32_kernel, dim3((unsigned)((n + 1023) / 1024)), dim3(256), 0, (hipStream_t)stream, in, out, n);
    return mh_check_launch("u8_to_f32");
}

// ---- Train.py's input side on the device (mh_frame_prepare): crop window + preprocessing.augment (Data_utils/preprocessing.py:31-89) + cast ----------------------
// The host uploads the decoded 8-bit frames as they are; sample b's window is cut out of its own source (zeros outside: the centre pad) and augmented with the
// fp32 operations of Data_utils/data_reader.augment in their order, UN-contracted (an fma would round once where numpy rounds twice): per pixel the result is the
// host's bit for bit, only the contrast mean is summed in another order (float64, two stages, fixed order).  A lane owns 4 consecutive window pixels = 12 source
// bytes (3 words where the address allows) = 3 float4 of each view and 1 float4 of the ground truth.
#if defined(__clang__)
#define MH_FP_EXACT _Pragma("clang fp contract(off)")
#else
#define MH_FP_EXACT
#endif
#define FP_SUM_PX 4096          // window pixels per workgroup of the partial-sum launch: 256 lanes x 4 quads of 4 pixels

struct FrameArgs { const mh_frame_seg* segs; float* left; float* right; float* gt; double* ws; int H, W, npix, nblk; };

// window pixels p0 .. p0+3 (p0 = y * W + x, p0 % 4 == 0, p0 < npix) of a uint8 [Hs][Ws][3] source -> 12 floats; 0 outside the source and past the window
__device__ __forceinline__ void frame_load4(const unsigned char* __restrict__ src, int Hs, int Ws, int r0, int c0, int W, int npix, int p0, int y, int x,
                                            float (&v)[12]) {
    const int sy = r0 + y, sx = c0 + x;
    if (x + 4 <= W && sy >= 0 && sy < Hs && sx >= 0 && sx + 4 <= Ws) {          // the four pixels are neighbours in one source row
        const unsigned char* q = src + ((int64_t)sy * Ws + sx) * 3;
        if ((((uintptr_t)q) & 3u) == 0) {
            const unsigned* q4 = reinterpret_cast<const unsigned*>(q);
            const unsigned w[3] = {q4[0], q4[1], q4[2]};
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                v[4 * k + 0] = (float)(w[k] & 0xffu); v[4 * k + 1] = (float)((w[k] >> 8) & 0xffu);
                v[4 * k + 2] = (float)((w[k] >> 16) & 0xffu); v[4 * k + 3] = (float)(w[k] >> 24);
            }
        } else {
#pragma unroll
            for (int k = 0; k < 12; ++k) v[k] = (float)q[k];
        }
        return;
    }
    int yy = y, xx = x;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        while (xx >= W) { xx -= W; ++yy; }
        const int ty = r0 + yy, tx = c0 + xx;
        const bool in = p0 + j < npix && ty >= 0 && ty < Hs && tx >= 0 && tx < Ws;
        const unsigned char* q = src + ((int64_t)(in ? ty : 0) * Ws + (in ? tx : 0)) * 3;
        v[3 * j + 0] = in ? (float)q[0] : 0.f; v[3 * j + 1] = in ? (float)q[1] : 0.f; v[3 * j + 2] = in ? (float)q[2] : 0.f;
        ++xx;
    }
}

// the ground truth of the same four pixels: float32, or uint16 / 256 (the KITTI disparity PNG; a division by a power of two: exact)
__device__ __forceinline__ void frame_load4_gt(const void* __restrict__ src, int kind, int Hs, int Ws, int r0, int c0, int W, int npix, int p0, int y, int x,
                                               float (&g)[4]) {
    const int sy = r0 + y, sx = c0 + x;
    if (x + 4 <= W && sy >= 0 && sy < Hs && sx >= 0 && sx + 4 <= Ws) {
        const int64_t e = (int64_t)sy * Ws + sx;
        if (kind) {
            const unsigned short* q = (const unsigned short*)src + e;
            if ((((uintptr_t)q) & 7u) == 0) {
                const uint2 w = *reinterpret_cast<const uint2*>(q);
                g[0] = (float)(w.x & 0xffffu) * (1.0f / 256.0f); g[1] = (float)(w.x >> 16) * (1.0f / 256.0f);
                g[2] = (float)(w.y & 0xffffu) * (1.0f / 256.0f); g[3] = (float)(w.y >> 16) * (1.0f / 256.0f);
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j) g[j] = (float)q[j] * (1.0f / 256.0f);
            }
        } else {
            const float* q = (const float*)src + e;
            if ((((uintptr_t)q) & 15u) == 0) {
                const float4 w = *reinterpret_cast<const float4*>(q);
                g[0] = w.x; g[1] = w.y; g[2] = w.z; g[3] = w.w;
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j) g[j] = q[j];
            }
        }
        return;
    }
    int yy = y, xx = x;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        while (xx >= W) { xx -= W; ++yy; }
        const int ty = r0 + yy, tx = c0 + xx;
        const bool in = p0 + j < npix && ty >= 0 && ty < Hs && tx >= 0 && tx < Ws;
        const int64_t e = in ? (int64_t)ty * Ws + tx : 0;
        g[j] = !in ? 0.f : kind ? (float)((const unsigned short*)src)[e] * (1.0f / 256.0f) : ((const float*)src)[e];
        ++xx;
    }
}

// one colour of tf.image.adjust_hue's way back: k = (6 h + off) mod 6 (6 h + off < 12), v - v s clip(min(k, 4 - k), 0, 1)
__device__ __forceinline__ float frame_hsv_channel(float h, float off, float v, float vs) {
    MH_FP_EXACT
    float k = h * 6.0f + off;
    k = k >= 6.0f ? k - 6.0f : k;                       // == fmodf(k, 6): exact
    const float t = fminf(fmaxf(fminf(k, 4.0f - k), 0.0f), 1.0f);
    return v - vs * t;
}

// preprocessing.augment on one pixel, as Data_utils/data_reader.augment states it; m = the three channel means of this view (read only with bit 1)
__device__ __forceinline__ void frame_augment(float& r, float& g, float& b, int active, float delta, float contrast, float hue, const float* m) {
    MH_FP_EXACT
    if (active & 1) { r = r + delta; g = g + delta; b = b + delta; }
    if (active & 2) {
        const float m0 = m[0], m1 = m[1], m2 = m[2];
        r = (r - m0) * contrast + m0; g = (g - m1) * contrast + m1; b = (b - m2) * contrast + m2;
    }
    if (active & 4) {
        const float mx = fmaxf(fmaxf(r, g), b), mn = fminf(fminf(r, g), b);
        const float d = mx - mn;
        const float s = mx > 0.f ? d / mx : 0.f;
        const float dd = d > 0.f ? d : 1.f;
        float h = (mx == r ? g - b : (mx == g ? b - r : r - g)) / dd;       // (one division: the three quotients of the host statement, selected first)
        h = mx == r ? h : (mx == g ? 2.0f + h : 4.0f + h);
        h = h / 6.0f;
        h = d > 0.f ? h - floorf(h) : 0.f;              // numpy's x % 1.0 for x > -1
        h = h + hue;
        h = h - floorf(h);
        const float vs = mx * s;
        r = frame_hsv_channel(h, 5.0f, mx, vs); g = frame_hsv_channel(h, 3.0f, mx, vs); b = frame_hsv_channel(h, 1.0f, mx, vs);
    }
    r = fminf(fmaxf(r, 0.f), 255.f); g = fminf(fmaxf(g, 0.f), 255.f); b = fminf(fmaxf(b, 0.f), 255.f);
}

// first launch (only with contrast): grid (nblk, 2 B); workgroup (i, 2 b + view) sums FP_SUM_PX window pixels of one view after the brightness step, per channel
__global__ __launch_bounds__(256) void frame_sums_kernel(FrameArgs a) {
    __shared__ double red[3][256];
    const int b = blockIdx.y >> 1, view = blockIdx.y & 1;
    const mh_frame_seg s = a.segs[b];
    if (!(s.active & 2)) return;                         // workgroup-uniform: nobody reads this sample's partial sums
    const unsigned char* src = (const unsigned char*)(view ? s.right : s.left);
    const bool bright = (s.active & 1) != 0;
    double acc[3] = {0.0, 0.0, 0.0};
    for (int i = 0; i < FP_SUM_PX / 1024; ++i) {
        const int p0 = ((int)blockIdx.x * (FP_SUM_PX / 4) + i * 256 + (int)threadIdx.x) * 4;
        if (p0 >= a.npix) break;
        const int y = p0 / a.W, x = p0 - y * a.W;
        float v[12];
        frame_load4(src, s.Hs, s.Ws, s.r0, s.c0, a.W, a.npix, p0, y, x, v);
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (p0 + j < a.npix) {
#pragma unroll
                for (int c = 0; c < 3; ++c) acc[c] += (double)(bright ? v[3 * j + c] + s.delta : v[3 * j + c]);
            }
    }
    red[0][threadIdx.x] = acc[0]; red[1][threadIdx.x] = acc[1]; red[2][threadIdx.x] = acc[2];
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) {
            red[0][threadIdx.x] += red[0][threadIdx.x + o];
            red[1][threadIdx.x] += red[1][threadIdx.x + o];
            red[2][threadIdx.x] += red[2][threadIdx.x + o];
        }
        __syncthreads();
    }
    if (threadIdx.x < 3) a.ws[((int64_t)blockIdx.y * a.nblk + blockIdx.x) * 3 + threadIdx.x] = red[threadIdx.x][0];
}

// the applying launch: grid (ceil(npix / 1024), B).  With contrast every workgroup first finishes its sample's six sums (view x channel) from the partial sums,
// 32 lanes per sum, in a fixed order.
__global__ __launch_bounds__(256) void frame_apply_kernel(FrameArgs a) {
    __shared__ double red[6][32];
    __shared__ float mean[6];
    const int b = blockIdx.y, t = threadIdx.x;
    const mh_frame_seg s = a.segs[b];
    const bool poison = (s.active & 2) && !a.ws;        // contrast without the partial sums: the caller broke its word -- say so in the result
    if ((s.active & 2) && a.ws) {
        const int j = t >> 5, l = t & 31;               // j = 3 * view + channel
        if (t < 192) {
            const double* part = a.ws + ((int64_t)(2 * b + j / 3) * a.nblk) * 3 + j % 3;
            double acc = 0.0;
            for (int i = l; i < a.nblk; i += 32) acc += part[(int64_t)i * 3];
            red[j][l] = acc;
        }
        __syncthreads();
        for (int o = 16; o > 0; o >>= 1) {
            if (t < 192 && l < o) red[j][l] += red[j][l + o];
            __syncthreads();
        }
        if (t < 6) mean[t] = (float)(red[t][0] / (double)a.npix);
        __syncthreads();
    }
    const int p0 = ((int)blockIdx.x * 256 + t) * 4;
    if (p0 >= a.npix) return;
    const int y = p0 / a.W, x = p0 - y * a.W;
    const bool full = p0 + 4 <= a.npix;
#pragma unroll
    for (int view = 0; view < 2; ++view) {
        float v[12];
        frame_load4((const unsigned char*)(view ? s.right : s.left), s.Hs, s.Ws, s.r0, s.c0, a.W, a.npix, p0, y, x, v);
#pragma unroll
        for (int j = 0; j < 4; ++j) frame_augment(v[3 * j], v[3 * j + 1], v[3 * j + 2], s.active, s.delta, s.contrast, s.hue, mean + 3 * view);
        if (poison) {
#pragma unroll
            for (int k = 0; k < 12; ++k) v[k] = __builtin_nanf("");
        }
        float* dst = (view ? a.right : a.left) + ((int64_t)b * a.npix + p0) * 3;
        if (full && (((uintptr_t)dst) & 15u) == 0) {
#pragma unroll
            for (int k = 0; k < 3; ++k) reinterpret_cast<float4*>(dst)[k] = make_float4(v[4 * k], v[4 * k + 1], v[4 * k + 2], v[4 * k + 3]);
        } else {
#pragma unroll
            for (int k = 0; k < 12; ++k) if (p0 + k / 3 < a.npix) dst[k] = v[k];
        }
    }
    float g[4];
    frame_load4_gt(s.gt, s.gt_kind, s.Hs, s.Ws, s.r0, s.c0, a.W, a.npix, p0, y, x, g);
    float* dst = a.gt + (int64_t)b * a.npix + p0;
    if (full && (((uintptr_t)dst) & 15u) == 0) {
        *reinterpret_cast<float4*>(dst) = make_float4(g[0], g[1], g[2], g[3]);
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) if (p0 + j < a.npix) dst[j] = g[j];
    }
}

static inline int frame_sum_blocks(int64_t npix) { return (int)((npix + FP_SUM_PX - 1) / FP_SUM_PX); }

extern "C" int64_t mh_frame_prepare_ws_floats(int32_t B, int32_t H, int32_t W) {
    if (B <= 0 || H <= 0 || W <= 0) return 0;
    return 2 * ((int64_t)B * 2 * frame_sum_blocks((int64_t)H * W) * 3);            // float64 partial sums: [B][view][workgroup][channel]
}

extern "C" int mh_frame_prepare(const mh_frame_seg* segs, int32_t B, int32_t H, int32_t W, float* left, float* right, float* gt, float* ws, void* stream) {
    MH_REQUIRE(segs && left && right && gt, MH_ERR_ARG, "mh_frame_prepare: null argument");
    MH_REQUIRE(B > 0 && H > 0 && W > 0, MH_ERR_ARG, "mh_frame_prepare: bad dimension");
    MH_REQUIRE((int64_t)H * W * 3 < (1ll << 31) && 2 * (int64_t)B < 65536, MH_ERR_UNSUPPORTED, "mh_frame_prepare: window or batch too large");
    MH_REQUIRE((((uintptr_t)ws) & 7u) == 0, MH_ERR_ALIGN, "mh_frame_prepare: ws must be 8-byte aligned");
    FrameArgs a{};
    a.segs = segs; a.left = left; a.right = right; a.gt = gt; a.ws = (double*)ws;
    a.H = H; a.W = W; a.npix = H * W; a.nblk = frame_sum_blocks(a.npix);
    if (ws) {
        hipLaunchKernelGGL(frame_sums_kernel, dim3((unsigned)a.nblk, (unsigned)(2 * B)), dim3(256), 0, (hipStream_t)stream, a);
        if (int e = mh_check_launch("frame_sums")) return e;
    }
    hipLaunchKernelGGL(frame_apply_kernel, dim3((unsigned)((a.npix + 1023) / 1024), (unsigned)B), dim3(256), 0, (hipStream_t)stream, a);
    mh_note_kernel("frame_apply_kernel grid %d x %d, %d launch%s", (a.npix + 1023) / 1024, B, ws ? 2 : 1, ws ? "es" : "");
    return mh_check_launch("frame_apply");
}

// ---- the live demo's input side: rectification of raw camera views (mh_rectify_map, mh_remap; the reference leaves it to the grabber, README.MD:97) ----------------
// mh_rectify_map: one lane per output pixel evaluates the formula of the header in its fp32 operations and their order, un-contracted, and stores one (x, y) pair
// (8 bytes per lane, consecutive lanes consecutive pairs).  The V camera records travel as kernel arguments: the wave reads them with scalar loads.
// mh_remap: a gather of a few MB that stays in L2 plus 12 bytes per pixel of writes.  A lane owns 4 consecutive output pixels = 2 float4 of the map and 3 float4 of
// the interleaved output, like frame_apply_kernel (a lane per pixel would store 3 dwords at a 12-byte stride); its 16 taps are single-element loads.
struct RectMapArgs { mh_camera_model cam[4]; float* map; int Wo, npix; };

__device__ __forceinline__ void rectify_point(const mh_camera_model& c, int u, int v, float& mx, float& my) {
    MH_FP_EXACT
    const float x = ((float)u - c.cxn) / c.fxn, y = ((float)v - c.cyn) / c.fyn;
    const float X = (c.R[0] * x + c.R[3] * y) + c.R[6];
    const float Y = (c.R[1] * x + c.R[4] * y) + c.R[7];
    const float W = (c.R[2] * x + c.R[5] * y) + c.R[8];
    const float xp = X / W, yp = Y / W;
    const float xx = xp * xp, yy = yp * yp, xy = xp * yp;
    const float r2 = xx + yy;
    const float r4 = r2 * r2;
    const float r6 = r4 * r2;
    const float rad = ((1.0f + c.k1 * r2) + c.k2 * r4) + c.k3 * r6;
    const float xd = (xp * rad + (2.0f * c.p1) * xy) + c.p2 * (r2 + 2.0f * xx);
    const float yd = (yp * rad + c.p1 * (r2 + 2.0f * yy)) + (2.0f * c.p2) * xy;
    mx = c.fx * xd + c.cx;
    my = c.fy * yd + c.cy;
    const bool ok = W > 0.f && fabsf(mx) <= 3.402823466e+38f && fabsf(my) <= 3.402823466e+38f;      // (NaN fails every comparison)
    if (!ok) { mx = -2.0f; my = -2.0f; }
}

// grid (ceil(npix / 256), V)
__global__ __launch_bounds__(256) void rectify_map_kernel(RectMapArgs a) {
    const int q = (int)blockIdx.x * 256 + (int)threadIdx.x;
    if (q >= a.npix) return;
    const int v = q / a.Wo, u = q - v * a.Wo;
    float mx, my;
    rectify_point(a.cam[blockIdx.y], u, v, mx, my);
    float* dst = a.map + ((int64_t)blockIdx.y * a.npix + q) * 2;
    if ((((uintptr_t)a.map) & 7u) == 0) {
        float2 pair;
        pair.x = mx; pair.y = my;
        *reinterpret_cast<float2*>(dst) = pair;
    } else { dst[0] = mx; dst[1] = my; }
}

struct RemapArgs { const void* src; const float* map; float* out; int Hs, Ws, Cs, u8, npix; };

// the three output channels of source pixel (y, x) of the view whose first pixel is `view_px`; 0 outside the source (the address is then the view's first pixel)
__device__ __forceinline__ void remap_tap(const RemapArgs& a, int64_t view_px, int y, int x, float (&s)[3]) {
    const bool in = x >= 0 && x < a.Ws && y >= 0 && y < a.Hs;
    const int64_t e = (view_px + (in ? (int64_t)y * a.Ws + x : 0)) * a.Cs;
    const int c1 = a.Cs > 1 ? 1 : 0, c2 = a.Cs > 1 ? 2 : 0;            // Cs = 1: the one channel three times; Cs = 4: the fourth is never read
    float r, g, b;
    if (a.u8) {
        const unsigned char* q = (const unsigned char*)a.src + e;
        r = (float)q[0]; g = (float)q[c1]; b = (float)q[c2];
    } else {
        const float* q = (const float*)a.src + e;
        r = q[0]; g = q[c1]; b = q[c2];
    }
    s[0] = in ? r : 0.f; s[1] = in ? g : 0.f; s[2] = in ? b : 0.f;
}

__device__ __forceinline__ void remap_pixel(const RemapArgs& a, int64_t view_px, float mx, float my, float* o) {
    MH_FP_EXACT
    o[0] = 0.f; o[1] = 0.f; o[2] = 0.f;
    if (!(mx > -1.0f && mx < (float)a.Ws && my > -1.0f && my < (float)a.Hs)) return;        // no tap inside (NaN and the (-2, -2) mark come here)
    const float x0f = floorf(mx), y0f = floorf(my);
    const float tx = mx - x0f, ty = my - y0f;
    const float ux = 1.0f - tx, uy = 1.0f - ty;
    const int x0 = (int)x0f, y0 = (int)y0f;
    float s00[3], s01[3], s10[3], s11[3];
    remap_tap(a, view_px, y0, x0, s00); remap_tap(a, view_px, y0, x0 + 1, s01);
    remap_tap(a, view_px, y0 + 1, x0, s10); remap_tap(a, view_px, y0 + 1, x0 + 1, s11);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float top = s00[c] * ux + s01[c] * tx;
        const float bot = s10[c] * ux + s11[c] * tx;
        o[c] = top * uy + bot * ty;
    }
}

// grid (ceil(npix / 1024), V)
__global__ __launch_bounds__(256) void remap_kernel(RemapArgs a) {
    const int p0 = ((int)blockIdx.x * 256 + (int)threadIdx.x) * 4;
    if (p0 >= a.npix) return;
    const int view = blockIdx.y;
    const bool full = p0 + 4 <= a.npix;
    const float* m = a.map + ((int64_t)view * a.npix + p0) * 2;
    float c[8];
    if (full && (((uintptr_t)m) & 15u) == 0) {
        const float4 m0 = reinterpret_cast<const float4*>(m)[0], m1 = reinterpret_cast<const float4*>(m)[1];
        c[0] = m0.x; c[1] = m0.y; c[2] = m0.z; c[3] = m0.w; c[4] = m1.x; c[5] = m1.y; c[6] = m1.z; c[7] = m1.w;
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const bool have = p0 + j < a.npix;
            c[2 * j] = have ? m[have ? 2 * j : 0] : -2.0f; c[2 * j + 1] = have ? m[have ? 2 * j + 1 : 0] : -2.0f;
        }
    }
    const int64_t view_px = (int64_t)view * a.Hs * a.Ws;
    float v[12];
#pragma unroll
    for (int j = 0; j < 4; ++j) remap_pixel(a, view_px, c[2 * j], c[2 * j + 1], v + 3 * j);
    float* dst = a.out + ((int64_t)view * a.npix + p0) * 3;
    if (full && (((uintptr_t)dst) & 15u) == 0) {
#pragma unroll
        for (int k = 0; k < 3; ++k) reinterpret_cast<float4*>(dst)[k] = make_float4(v[4 * k], v[4 * k + 1], v[4 * k + 2], v[4 * k + 3]);
    } else {
#pragma unroll
        for (int k = 0; k < 12; ++k) if (p0 + k / 3 < a.npix) dst[k] = v[k];
    }
}

static inline bool rectify_focal_ok(float f) { return f != 0.f && f == f && fabsf(f) <= 3.402823466e+38f; }

extern "C" int mh_rectify_map(const mh_camera_model* cams, int32_t V, int32_t Ho, int32_t Wo, float* map, void* stream) {
    MH_REQUIRE(cams && map, MH_ERR_ARG, "mh_rectify_map: null argument");
    MH_REQUIRE(V >= 1 && V <= 4, MH_ERR_ARG, "mh_rectify_map: V = %d outside 1..4", V);
    MH_REQUIRE(Ho > 0 && Wo > 0, MH_ERR_ARG, "mh_rectify_map: bad dimension");
    for (int i = 0; i < V; ++i)
        MH_REQUIRE(rectify_focal_ok(cams[i].fx) && rectify_focal_ok(cams[i].fy) && rectify_focal_ok(cams[i].fxn) && rectify_focal_ok(cams[i].fyn), MH_ERR_ARG,
                   "mh_rectify_map: view %d has a zero or non-finite focal length", i);
    MH_REQUIRE((int64_t)Ho * Wo * 3 < (1ll << 31), MH_ERR_UNSUPPORTED, "mh_rectify_map: output too large");
    RectMapArgs a{};
    for (int i = 0; i < V; ++i) a.cam[i] = cams[i];
    a.map = map; a.Wo = Wo; a.npix = Ho * Wo;
    hipLaunchKernelGGL(rectify_map_kernel, dim3((unsigned)((a.npix + 255) / 256), (unsigned)V), dim3(256), 0, (hipStream_t)stream, a);
    mh_note_kernel("rectify_map_kernel grid %d x %d", (a.npix + 255) / 256, V);
    return mh_check_launch("rectify_map");
}

extern "C" int mh_remap(const void* src, int32_t src_u8, const float* map, float* out, int32_t V, int32_t Hs, int32_t Ws, int32_t Cs, int32_t Ho, int32_t Wo,
                        void* stream) {
    MH_REQUIRE(src && map && out, MH_ERR_ARG, "mh_remap: null argument");
    MH_REQUIRE(V >= 1 && V <= 4, MH_ERR_ARG, "mh_remap: V = %d outside 1..4", V);
    MH_REQUIRE(Hs > 0 && Ws > 0 && Ho > 0 && Wo > 0, MH_ERR_ARG, "mh_remap: bad dimension");
    MH_REQUIRE(Cs == 1 || Cs == 3 || Cs == 4, MH_ERR_ARG, "mh_remap: Cs = %d is not 1, 3 or 4", Cs);
    MH_REQUIRE((int64_t)Hs * Ws <= (1ll << 31) / (V * Cs), MH_ERR_ARG, "mh_remap: more than 2^31 source elements");
    MH_REQUIRE((int64_t)Ho * Wo * 3 < (1ll << 31), MH_ERR_UNSUPPORTED, "mh_remap: output too large");
    RemapArgs a{};
    a.src = src; a.map = map; a.out = out; a.Hs = Hs; a.Ws = Ws; a.Cs = Cs; a.u8 = src_u8 != 0; a.npix = Ho * Wo;
    hipLaunchKernelGGL(remap_kernel, dim3((unsigned)((a.npix + 1023) / 1024), (unsigned)V), dim3(256), 0, (hipStream_t)stream, a);
    mh_note_kernel("remap_kernel grid %d x %d", (a.npix + 1023) / 1024, V);
    return mh_check_launch("remap");
}

// ---- proxy labels of the continual loop on the device (mh_sgm_proxy, mh_sgm_proxy_ex): census + four- or eight-path semi-global matching, 3x3 median --------------
// Replaces the proxy column of the continual list (an external matcher's PNGs).  Integer arithmetic up to the sub-pixel step, no atomics, every launch writes
// what the next one reads: the result does not depend on launch shape or order.  Workspace: census words [2][B][H][W] (8 bytes), one uint8 volume [B][H][W][D]
// per path (L_r <= 64 + p2 <= 255), the right view's winner [B][H][W] (uint8).  The matching cost is never stored: a path step recomputes
// popcount(cL(y, x) ^ cR(y, x - d)) from the census rows (16 bytes per pixel and view instead of a D-byte volume read by four paths).
// mh_sgm_proxy_ex: P = 4 or 8 volumes (the four diagonals behind the four axis paths; the kernels are templated on P); for P = 8 one more pass folds the eight
// volumes into their sum S, uint16 [B][H][W][D] behind the volumes, which the right-view and select kernels read instead (the right-view walk gathers single
// elements, and gathered from eight volumes it took 7.26 ms at 375 x 1242, D = 128, against 1.05 ms from four: profiles/sgm_proxy.txt); with the median the
// labels before the filter, float [B][H][W], lie behind the right view's winners.
// mh_sgm_proxy_scaled, scale 2: the same launches on the half grays [2][B][h][w] that sgm_half_gray_kernel writes in front of this workspace (the census then
// reads a single channel: sgm_census_kernel<1>), and sgm_upsample2_kernel doubles the half-resolution labels behind it into `proxy`.
#define SGM_BIG (1 << 20)
#define SGM_CT_W 32             // census tile: 32 x 8 pixels per workgroup, halo 4 x 3
#define SGM_CT_H 8

struct SgmArgs {
    const void* left; const void* right;
    unsigned long long* census; unsigned char* vol; unsigned short* fold; unsigned char* dr; float* out;      // fold: P = 8 only; out: what sgm_select_kernel writes (proxy, or the map in front of the median)
    int64_t vstride;            // bytes between two path volumes
    int B, H, W, D, u8, p1, p2, uniq, lr_tol, npix;
};

// integers through the float shuffle (the bits travel unchanged); the mask may differ per lane
__device__ __forceinline__ int sgm_shfl_xor(int v, int mask) { return __builtin_bit_cast(int, __shfl_xor(__builtin_bit_cast(float, v), mask)); }
__device__ __forceinline__ int sgm_wave_min(int v) {
    v = min(v, sgm_shfl_xor(v, 32)); v = min(v, sgm_shfl_xor(v, 16)); v = min(v, sgm_shfl_xor(v, 8));
    v = min(v, sgm_shfl_xor(v, 4)); v = min(v, sgm_shfl_xor(v, 2)); v = min(v, sgm_shfl_xor(v, 1));
    return v;
}
__device__ __forceinline__ int sgm_u8(float v) { return (int)fminf(fmaxf(floorf(v + 0.5f), 0.f), 255.f); }

// gray + census 9 x 7 of both views: grid (tiles x, tiles y, 2 B), z = 2 b + view.  GRAY = 0: the sources are [B,H,W,3] frames, uint8 or float32 (a.u8);
// GRAY = 1: they are [B,H,W] uint8 gray images (the half grays of mh_sgm_proxy_scaled) and are taken as they are
template <int GRAY>
__global__ __launch_bounds__(256) void sgm_census_kernel(SgmArgs a) {
    __shared__ int s_g[SGM_CT_H + 6][SGM_CT_W + 8];
    const int b = (int)blockIdx.z >> 1, view = (int)blockIdx.z & 1;
    const int x0 = (int)blockIdx.x * SGM_CT_W, y0 = (int)blockIdx.y * SGM_CT_H;
    const void* src = view ? a.right : a.left;
    const int64_t frame = (int64_t)b * a.H * a.W;
    for (int i = threadIdx.x; i < (SGM_CT_H + 6) * (SGM_CT_W + 8); i += 256) {
        const int ty = i / (SGM_CT_W + 8), tx = i - ty * (SGM_CT_W + 8);
        const int y = min(max(y0 + ty - 3, 0), a.H - 1), x = min(max(x0 + tx - 4, 0), a.W - 1);
        if (GRAY) { s_g[ty][tx] = ((const unsigned char*)src)[frame + (int64_t)y * a.W + x]; continue; }
        const int64_t e = (frame + (int64_t)y * a.W + x) * 3;
        int r, g, bl;
        if (a.u8) {
            const unsigned char* q = (const unsigned char*)src + e;
            r = q[0]; g = q[1]; bl = q[2];
        } else {
            const float* q = (const float*)src + e;
            r = sgm_u8(q[0]); g = sgm_u8(q[1]); bl = sgm_u8(q[2]);
        }
        s_g[ty][tx] = (77 * r + 150 * g + 29 * bl + 128) >> 8;
    }
    __syncthreads();
    const int tx = threadIdx.x & (SGM_CT_W - 1), ty = threadIdx.x / SGM_CT_W;
    const int x = x0 + tx, y = y0 + ty;
    if (x >= a.W || y >= a.H) return;
    const int c = s_g[ty + 3][tx + 4];
    unsigned w0 = 0, w1 = 0;
    int k = 0;
#pragma unroll
    for (int dy = 0; dy < 7; ++dy) {
#pragma unroll
        for (int dx = 0; dx < 9; ++dx) {
            if (dy == 3 && dx == 4) continue;
            const unsigned bit = s_g[ty + dy][tx + dx] < c ? 1u : 0u;
            if (k < 31) w0 = (w0 << 1) | bit; else w1 = (w1 << 1) | bit;
            ++k;
        }
    }
    a.census[(int64_t)view * a.npix + frame + (int64_t)y * a.W + x] = ((unsigned long long)w0 << 32) | w1;
}

// the costs of this lane's K disparities (d = K lane + k) at pixel x of a row: cl = the left word, cr = the right view's row
template <int K>
__device__ __forceinline__ void sgm_cost(const unsigned long long* __restrict__ cr, unsigned long long cl, int x, int lane, int (&c)[K]) {
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const int xr = x - (lane * K + k);
        const int h = __builtin_popcountll(cl ^ cr[max(xr, 0)]);           // (the load is unconditional: nothing waits for it at a branch join)
        c[k] = xr >= 0 ? h : 64;
    }
}

// Aggregation, all P paths in one launch: grid (2 H + 2 W [+ 4 (H + W - 1)], B), one wave per path line -- a row left->right / right->left, a column top->bottom /
// bottom->top, and for P = 8 the diagonals (dy, dx) = (+1,+1), (+1,-1), (-1,+1), (-1,-1): a line starts at every pixel whose predecessor lies outside the frame
// (line j < W at column j of the first row in walking order, the others at the rows behind it on the side the walk comes from) and runs until it leaves the
// frame --, K = D / 64 neighbouring disparities per lane: d -/+ 1 come from the neighbouring lane, m from a wave min.  Sequential along the line (the
// step's chain is two shuffles + the six of the reduction), parallel across lines and paths; the next pixel's costs are fetched before the step.
template <int K, int P>
__global__ __launch_bounds__(64) void sgm_paths_kernel(SgmArgs a) {
    const int lane = threadIdx.x, b = blockIdx.y;
    int line = blockIdx.x, path, y, x, dy = 0, dx = 0, n;
    if (line < 2 * a.H) { path = line & 1; y = line >> 1; x = path ? a.W - 1 : 0; dx = path ? -1 : 1; n = a.W; }
    else if (P == 4 || line < 2 * a.H + 2 * a.W) { line -= 2 * a.H; path = 2 + (line & 1); x = line >> 1; y = (line & 1) ? a.H - 1 : 0; dy = (line & 1) ? -1 : 1; n = a.H; }
    else {
        line -= 2 * a.H + 2 * a.W;
        const int per = a.H + a.W - 1, dir = line / per, j = line - dir * per, t = j - a.W + 1;      // t >= 1: the line starts in row t of the walk, at the side
        path = 4 + dir; dy = (dir & 2) ? -1 : 1; dx = (dir & 1) ? -1 : 1;
        const int row = t > 0 ? t : 0;
        y = dy > 0 ? row : a.H - 1 - row;
        x = t > 0 ? (dx > 0 ? 0 : a.W - 1) : j;
        n = min(dy > 0 ? a.H - y : y + 1, dx > 0 ? a.W - x : x + 1);
    }
    const int64_t frame = (int64_t)b * a.H * a.W;
    const unsigned long long* __restrict__ cl = a.census + frame;
    const unsigned long long* __restrict__ cr = a.census + a.npix + frame;
    unsigned char* __restrict__ vol = a.vol + (int64_t)path * a.vstride + frame * a.D + lane * K;
    const int up_mask = lane < 63 ? (lane ^ (lane + 1)) : 0;           // lane ^ mask = lane + 1
    int L[K], c[K], cn[K], m = 0;
    sgm_cost<K>(cr + (int64_t)y * a.W, cl[(int64_t)y * a.W + x], x, lane, c);
    for (int i = 0; i < n; ++i) {
        const int yn = y + dy, xn = x + dx;
        const int yf = min(max(yn, 0), a.H - 1), xf = min(max(xn, 0), a.W - 1);        // the line's last step fetches its own pixel again
        sgm_cost<K>(cr + (int64_t)yf * a.W, cl[(int64_t)yf * a.W + xf], xf, lane, cn);
        int mn = SGM_BIG;
        if (i == 0) {
#pragma unroll
            for (int k = 0; k < K; ++k) { L[k] = c[k]; mn = min(mn, L[k]); }
        } else {
            int below = __shfl_up(L[K - 1], 1u), above = sgm_shfl_xor(L[0], up_mask);
            if (lane == 0) below = SGM_BIG;                            // d - 1 < 0 and d + 1 > D - 1: absent
            if (lane == 63) above = SGM_BIG;
            int nl[K];
#pragma unroll
            for (int k = 0; k < K; ++k) {
                const int lo = k ? L[k - 1] : below, hi = k < K - 1 ? L[k + 1] : above;
                nl[k] = c[k] + min(min(L[k], min(lo, hi) + a.p1), m + a.p2) - m;
                mn = min(mn, nl[k]);
            }
#pragma unroll
            for (int k = 0; k < K; ++k) L[k] = nl[k];
        }
        m = sgm_wave_min(mn);
        unsigned char* q = vol + ((int64_t)y * a.W + x) * a.D;
        if (K == 2) *reinterpret_cast<unsigned short*>(q) = (unsigned short)(L[0] | (L[K - 1] << 8));
        else {
#pragma unroll
            for (int k = 0; k < K; ++k) q[k] = (unsigned char)L[k];
        }
#pragma unroll
        for (int k = 0; k < K; ++k) c[k] = cn[k];
        y = yn; x = xn;
    }
}

// S(pixel, d) = the sum of the four paths; p points at path 0's byte
__device__ __forceinline__ int sgm_sum4(const unsigned char* __restrict__ p, int64_t vs) { return (int)p[0] + (int)p[vs] + (int)p[2 * vs] + (int)p[3 * vs]; }

// P = 8: S = the sum of the eight volumes, once, as uint16 (S <= 2040).  One thread per 8 neighbouring elements: eight 8-byte loads, one 16-byte store
__global__ __launch_bounds__(256) void sgm_fold_kernel(SgmArgs a, int64_t n8) {
    const int64_t i = (int64_t)blockIdx.x * 256 + (int64_t)threadIdx.x;
    if (i >= n8) return;
    int s[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int p = 0; p < 8; ++p) {
        const unsigned long long w = *reinterpret_cast<const unsigned long long*>(a.vol + p * a.vstride + i * 8);
#pragma unroll
        for (int k = 0; k < 8; ++k) s[k] += (int)((w >> (8 * k)) & 255u);
    }
    unsigned long long o[2];
#pragma unroll
    for (int h = 0; h < 2; ++h)
        o[h] = (unsigned long long)s[4 * h] | ((unsigned long long)s[4 * h + 1] << 16) | ((unsigned long long)s[4 * h + 2] << 32) | ((unsigned long long)s[4 * h + 3] << 48);
    unsigned long long* q = reinterpret_cast<unsigned long long*>(a.fold + i * 8);
    q[0] = o[0]; q[1] = o[1];
}

// the right view's winner from the same volume: dR(y, x') = argmin over d with x' + d < W of S(y, x' + d, d), lowest d on ties.  One lane per pixel walks the diagonal
template <int P>
__global__ __launch_bounds__(256) void sgm_right_kernel(SgmArgs a) {
    const int pix = (int)blockIdx.x * 256 + (int)threadIdx.x;
    if (pix >= a.npix) return;
    const int x = pix % a.W, nd = min(a.D, a.W - x);
    const unsigned char* __restrict__ p = a.vol + (int64_t)pix * a.D;
    const unsigned short* __restrict__ f = a.fold + (int64_t)pix * a.D;
    int best = SGM_BIG, bd = 0;
#pragma unroll 4
    for (int d = 0; d < nd; ++d) {
        const int s = P == 8 ? (int)f[(int64_t)d * (a.D + 1)] : sgm_sum4(p + (int64_t)d * (a.D + 1), a.vstride);
        if (s < best) { best = s; bd = d; }
    }
    a.dr[pix] = (unsigned char)bd;
}

// winner, uniqueness, left-right check, sub-pixel: one wave per pixel (4 per workgroup), K disparities per lane.  Every pixel is written (0 = rejected)
template <int K, int P>
__global__ __launch_bounds__(256) void sgm_select_kernel(SgmArgs a) {
    const int lane = threadIdx.x & 63, pix = (int)blockIdx.x * 4 + ((int)threadIdx.x >> 6);
    if (pix >= a.npix) return;                                          // wave-uniform
    const unsigned char* __restrict__ p = a.vol + (int64_t)pix * a.D + lane * K;
    const unsigned short* __restrict__ f = a.fold + (int64_t)pix * a.D + lane * K;
    int S[K], key = 0x7fffffff;
#pragma unroll
    for (int k = 0; k < K; ++k) { S[k] = P == 8 ? (int)f[k] : sgm_sum4(p + k, a.vstride); key = min(key, (S[k] << 8) | (lane * K + k)); }      // S <= 255 P <= 2040, d < 256: lowest d on ties
    key = sgm_wave_min(key);
    const int d1 = key & 255, s1 = key >> 8;
    int s2 = SGM_BIG, sm = SGM_BIG, sp = SGM_BIG;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const int d = lane * K + k;
        if (d < d1 - 1 || d > d1 + 1) s2 = min(s2, S[k]);
        if (d == d1 - 1) sm = S[k];
        if (d == d1 + 1) sp = S[k];
    }
    s2 = sgm_wave_min(s2); sm = sgm_wave_min(sm); sp = sgm_wave_min(sp);
    if (lane) return;
    bool ok = !(s2 < SGM_BIG && a.uniq * s2 < 100 * s1) && d1 != 0;
    const int xr = pix % a.W - d1;
    ok = ok && xr >= 0;
    if (ok) { const int back = a.dr[pix - d1]; ok = abs(back - d1) <= a.lr_tol; }
    float o = (float)d1;
    if (d1 >= 1 && d1 <= a.D - 2) {
        const int den = 2 * (sm + sp - 2 * s1);
        if (den > 0) o = o + (float)(sm - sp) / (float)den;
    }
    a.out[pix] = ok ? o : 0.f;
}

// 3x3 median of the finished label map, one thread per pixel: a rejected pixel (0) stays 0, a valid one becomes the lower median -- index (n - 1) / 2 of the n valid
// values in ascending order -- of the valid labels among its neighbours inside its own frame.  A copy of one input value.  No sorting network and no register
// array indexed at run time: a label that is absent counts as +inf, every candidate counts the candidates that sort before it (ties by position), and the one
// whose count is (n - 1) / 2 is kept; n >= 1 makes that one a valid label.
__global__ __launch_bounds__(256) void sgm_median_kernel(const float* __restrict__ in, float* __restrict__ out, int H, int W, int npix) {
    const int pix = (int)blockIdx.x * 256 + (int)threadIdx.x;
    if (pix >= npix) return;
    const int x = pix % W, y = (pix / W) % H;
    float v[9];
    int n = 0;
#pragma unroll
    for (int i = 0; i < 9; ++i) {
        const int oy = i / 3 - 1, ox = i % 3 - 1;
        const bool inside = y + oy >= 0 && y + oy < H && x + ox >= 0 && x + ox < W;
        const float t = in[pix + (inside ? oy * W + ox : 0)];
        const bool valid = inside && t > 0.f;
        v[i] = valid ? t : __builtin_inff();
        n += valid ? 1 : 0;
    }
    const int want = (n - 1) >> 1;
    float r = 0.f;
#pragma unroll
    for (int i = 0; i < 9; ++i) {
        int before = 0;
#pragma unroll
        for (int j = 0; j < 9; ++j)
            if (j != i) before += (v[j] < v[i] || (v[j] == v[i] && j < i)) ? 1 : 0;
        if (before == want) r = v[i];
    }
    out[pix] = v[4] < __builtin_inff() ? r : 0.f;
}

// ---- mh_sgm_proxy_scaled, scale 2: the half grays in front of the matcher, the doubled labels behind it ----------------------------------------------------------------
// the matcher's gray of one full-resolution pixel (as sgm_census_kernel<0> computes it); e = the index of its first channel
__device__ __forceinline__ int sgm_gray_px(const void* __restrict__ src, int u8, int64_t e) {
    int r, g, bl;
    if (u8) {
        const unsigned char* q = (const unsigned char*)src + e;
        r = q[0]; g = q[1]; bl = q[2];
    } else {
        const float* q = (const float*)src + e;
        r = sgm_u8(q[0]); g = sgm_u8(q[1]); bl = sgm_u8(q[2]);
    }
    return (77 * r + 150 * g + 29 * bl + 128) >> 8;
}

// g2 [2][B][h][w] (uint8) = the rounded 2 x 2 mean of the gray frame, both views and all images in one launch: grid (cdiv(h w, 256), 2 B), y = 2 b + view, one
// thread per half pixel in row-major order.  Neighbouring lanes read neighbouring 6-byte (uint8) or 24-byte (float32) pieces of two source rows and store
// neighbouring bytes; the last column of an odd W and the last row of an odd H read their own pixel twice.
__global__ __launch_bounds__(256) void sgm_half_gray_kernel(const void* __restrict__ left, const void* __restrict__ right, unsigned char* __restrict__ g2,
                                                            int B, int H, int W, int h, int w, int u8) {
    const int p = (int)blockIdx.x * 256 + (int)threadIdx.x;
    if (p >= h * w) return;
    const int b = (int)blockIdx.y >> 1, view = (int)blockIdx.y & 1;
    const void* src = view ? right : left;
    const int y = p / w, x = p - y * w;
    const int xa = 2 * x, xb = min(2 * x + 1, W - 1), ya = 2 * y, yb = min(2 * y + 1, H - 1);
    const int64_t ra = ((int64_t)b * H + ya) * W, rb = ((int64_t)b * H + yb) * W;
    const int s = sgm_gray_px(src, u8, (ra + xa) * 3) + sgm_gray_px(src, u8, (ra + xb) * 3) + sgm_gray_px(src, u8, (rb + xa) * 3) + sgm_gray_px(src, u8, (rb + xb) * 3);
    g2[((int64_t)view * B + b) * h * w + p] = (unsigned char)((s + 2) >> 2);
}

__device__ __forceinline__ float sgm_up2(float l) { return l > 0.f ? 2.f * l : 0.f; }

// proxy(b, y, x) = 2 l(b, y >> 1, x >> 1) where that label is > 0, else 0: grid (cdiv(W / 4 + 2, 64), cdiv(H, 4), B), 64 pieces x 4 rows per workgroup.  A row of
// `proxy` starts anywhere (odd W, a caller's offset), so piece 0 is the `lead` floats in front of the row's first 16-byte boundary, written one by one, piece q >= 1
// the four floats behind them at lead + 4 (q - 1), one 16-byte store, and the piece the row's end cuts is written one by one again.  A piece that starts at an odd
// column takes three half labels, else two; the last row of an odd H reads row h - 1 like every other: y >> 1.
__global__ __launch_bounds__(256) void sgm_upsample2_kernel(const float* __restrict__ lab, float* __restrict__ proxy, int H, int W, int h, int w) {
    const int q = (int)blockIdx.x * 64 + ((int)threadIdx.x & 63), y = (int)blockIdx.y * 4 + ((int)threadIdx.x >> 6), b = (int)blockIdx.z;
    if (y >= H) return;
    float* __restrict__ row = proxy + ((int64_t)b * H + y) * W;
    const float* __restrict__ src = lab + ((int64_t)b * h + (y >> 1)) * w;
    const int lead = (int)((4u - (unsigned)(((uintptr_t)row >> 2) & 3u)) & 3u);
    if (q == 0) {
        for (int x = 0; x < min(lead, W); ++x) row[x] = sgm_up2(src[x >> 1]);
        return;
    }
    const int64_t c64 = (int64_t)lead + 4 * (int64_t)(q - 1);
    if (c64 >= W) return;
    const int c = (int)c64;
    if (c + 4 <= W) {
        *reinterpret_cast<float4*>(row + c) = make_float4(sgm_up2(src[c >> 1]), sgm_up2(src[(c + 1) >> 1]), sgm_up2(src[(c + 2) >> 1]), sgm_up2(src[(c + 3) >> 1]));
    } else {
        for (int x = c; x < W; ++x) row[x] = sgm_up2(src[x >> 1]);
    }
}

static inline int64_t sgm_align16(int64_t n) { return (n + 15) / 16 * 16; }

extern "C" int64_t mh_sgm_ws_bytes_ex(int32_t B, int32_t H, int32_t W, int32_t D, int32_t paths, int32_t median) {
    if (B <= 0 || H <= 0 || W <= 0 || D <= 0 || (paths != 4 && paths != 8) || (median != 0 && median != 1)) return 0;
    const int64_t npix = (int64_t)B * H * W;
    return sgm_align16(2 * npix * 8) + paths * sgm_align16(npix * D) + (paths == 8 ? sgm_align16(npix * D * 2) : 0) + sgm_align16(npix)
           + (median ? sgm_align16(npix * 4) : 0);
}

extern "C" int64_t mh_sgm_ws_bytes(int32_t B, int32_t H, int32_t W, int32_t D) { return mh_sgm_ws_bytes_ex(B, H, W, D, 4, 0); }

// census, aggregation, right view, select of one call: K = D / 64 disparities per lane, P paths; gray: the sources are [B,H,W] uint8 gray images
template <int K, int P>
static int sgm_launch(const SgmArgs& a, bool gray, hipStream_t s) {
    const int64_t npix = a.npix;
    const dim3 cgrid((unsigned)mh_cdiv(a.W, SGM_CT_W), (unsigned)mh_cdiv(a.H, SGM_CT_H), (unsigned)(2 * a.B));
    if (gray) hipLaunchKernelGGL(sgm_census_kernel<1>, cgrid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL(sgm_census_kernel<0>, cgrid, dim3(256), 0, s, a);
    if (int e = mh_check_launch("sgm_census")) return e;
    const int nlines = 2 * a.H + 2 * a.W + (P == 8 ? 4 * (a.H + a.W - 1) : 0);
    hipLaunchKernelGGL((sgm_paths_kernel<K, P>), dim3((unsigned)nlines, (unsigned)a.B), dim3(64), 0, s, a);
    if (int e = mh_check_launch("sgm_paths")) return e;
    if (P == 8) {
        const int64_t n8 = npix * a.D / 8;                              // D is a multiple of 64; < 2^31 * 24
        hipLaunchKernelGGL(sgm_fold_kernel, dim3((unsigned)mh_cdiv(n8, 256)), dim3(256), 0, s, a, n8);
        if (int e = mh_check_launch("sgm_fold")) return e;
    }
    hipLaunchKernelGGL(sgm_right_kernel<P>, dim3((unsigned)mh_cdiv(npix, 256)), dim3(256), 0, s, a);
    if (int e = mh_check_launch("sgm_right")) return e;
    hipLaunchKernelGGL((sgm_select_kernel<K, P>), dim3((unsigned)mh_cdiv(npix, 4)), dim3(256), 0, s, a);
    mh_note_kernel("sgm_paths_kernel<%d, %d> grid %d x %d", K, P, nlines, a.B);
    return mh_check_launch("sgm_select");
}

// the argument checks of every entry, nothing launched; `who` names the entry in the messages.  left / right / ws / proxy, H, W, D: what the matcher itself is given
// (at scale 2 the half grays, the half frame, D / 2)
static int sgm_check(const char* who, const void* left, const void* right, const void* ws, const float* proxy, int32_t B, int32_t H, int32_t W, int32_t D,
                     int32_t p1, int32_t p2, int32_t uniq, int32_t lr_tol, int32_t paths, int32_t median) {
    MH_REQUIRE(left && right && ws && proxy, MH_ERR_ARG, "%s: null argument", who);
    MH_REQUIRE(B > 0 && H > 0 && W > 0, MH_ERR_ARG, "%s: bad dimension", who);
    MH_REQUIRE(H >= 7 && W >= 9, MH_ERR_ARG, "%s: the frame must hold one census window (H >= 7, W >= 9)", who);
    MH_REQUIRE(D >= 1 && D <= 192 && D % 64 == 0, MH_ERR_UNSUPPORTED, "%s: D must be 64, 128 or 192", who);
    MH_REQUIRE(p1 > 0 && p1 <= p2, MH_ERR_ARG, "%s: penalties must satisfy 0 < p1 <= p2", who);
    MH_REQUIRE(64 + p2 <= 255, MH_ERR_ARG, "%s: 64 + p2 must fit 8 bits (the path volumes are uint8)", who);
    MH_REQUIRE(uniq > 0 && uniq <= 100, MH_ERR_ARG, "%s: uniq must lie in 1 .. 100", who);
    MH_REQUIRE(lr_tol >= 0, MH_ERR_ARG, "%s: lr_tol must not be negative", who);
    MH_REQUIRE(paths == 4 || paths == 8, MH_ERR_ARG, "%s: paths must be 4 or 8", who);
    MH_REQUIRE(median == 0 || median == 1, MH_ERR_ARG, "%s: median must be 0 or 1", who);
    MH_REQUIRE(mh_aligned16(ws), MH_ERR_ALIGN, "%s: ws must be 16-byte aligned", who);
    MH_REQUIRE((int64_t)B * H * W < (1ll << 31) - 256 && B < 32768 && H < 65536 * SGM_CT_H, MH_ERR_UNSUPPORTED, "%s: too many pixels or frames", who);
    return MH_OK;
}

// the matcher's launches on checked arguments.  gray: left, right are [B,H,W] uint8 gray images
static int sgm_run(const void* left, const void* right, int32_t frames_u8, bool gray, void* ws, float* proxy, int32_t B, int32_t H, int32_t W, int32_t D,
                   int32_t p1, int32_t p2, int32_t uniq, int32_t lr_tol, int32_t paths, int32_t median, void* stream) {
    SgmArgs a{};
    const int64_t npix = (int64_t)B * H * W;
    a.left = left; a.right = right;
    a.census = (unsigned long long*)ws;
    a.vol = (unsigned char*)ws + sgm_align16(2 * npix * 8);
    a.vstride = sgm_align16(npix * D);
    a.fold = (unsigned short*)(a.vol + paths * a.vstride);             // read only by the P = 8 kernels
    a.dr = a.vol + paths * a.vstride + (paths == 8 ? sgm_align16(npix * D * 2) : 0);
    float* raw = (float*)(a.dr + sgm_align16(npix));                   // the labels in front of the median (only with median)
    a.out = median ? raw : proxy;
    a.B = B; a.H = H; a.W = W; a.D = D; a.u8 = frames_u8 ? 1 : 0; a.p1 = p1; a.p2 = p2; a.uniq = uniq; a.lr_tol = lr_tol; a.npix = (int)npix;
    hipStream_t s = (hipStream_t)stream;
    int e;
    switch (D / 64 * 16 + paths) {
        case 16 + 4: e = sgm_launch<1, 4>(a, gray, s); break;
        case 32 + 4: e = sgm_launch<2, 4>(a, gray, s); break;
        case 48 + 4: e = sgm_launch<3, 4>(a, gray, s); break;
        case 16 + 8: e = sgm_launch<1, 8>(a, gray, s); break;
        case 32 + 8: e = sgm_launch<2, 8>(a, gray, s); break;
        default: e = sgm_launch<3, 8>(a, gray, s); break;
    }
    if (e || !median) return e;
    hipLaunchKernelGGL(sgm_median_kernel, dim3((unsigned)mh_cdiv(npix, 256)), dim3(256), 0, s, (const float*)raw, proxy, H, W, (int)npix);
    return mh_check_launch("sgm_median");
}

// the one host function behind the full-resolution entries
static int sgm_proxy_impl(const char* who, const void* left, const void* right, int32_t frames_u8, void* ws, float* proxy, int32_t B, int32_t H, int32_t W, int32_t D,
                          int32_t p1, int32_t p2, int32_t uniq, int32_t lr_tol, int32_t paths, int32_t median, void* stream) {
    if (int e = sgm_check(who, left, right, ws, proxy, B, H, W, D, p1, p2, uniq, lr_tol, paths, median)) return e;
    return sgm_run(left, right, frames_u8, false, ws, proxy, B, H, W, D, p1, p2, uniq, lr_tol, paths, median, stream);
}

extern "C" int mh_sgm_proxy_ex(const void* left, const void* right, int32_t frames_u8, void* ws, float* proxy, int32_t B, int32_t H, int32_t W, int32_t D,
                               int32_t p1, int32_t p2, int32_t uniq, int32_t lr_tol, int32_t paths, int32_t median, void* stream) {
    return sgm_proxy_impl("mh_sgm_proxy_ex", left, right, frames_u8, ws, proxy, B, H, W, D, p1, p2, uniq, lr_tol, paths, median, stream);
}

extern "C" int mh_sgm_proxy(const void* left, const void* right, int32_t frames_u8, void* ws, float* proxy, int32_t B, int32_t H, int32_t W, int32_t D,
                            int32_t p1, int32_t p2, int32_t uniq, int32_t lr_tol, void* stream) {
    return sgm_proxy_impl("mh_sgm_proxy", left, right, frames_u8, ws, proxy, B, H, W, D, p1, p2, uniq, lr_tol, 4, 0, stream);
}

// scale 1: mh_sgm_ws_bytes_ex; scale 2 (D = the full-resolution range): half grays | the matcher's workspace on the half frame | half-resolution labels
extern "C" int64_t mh_sgm_ws_bytes_scaled(int32_t B, int32_t H, int32_t W, int32_t D, int32_t paths, int32_t median, int32_t scale) {
    if (scale == 1) return mh_sgm_ws_bytes_ex(B, H, W, D, paths, median);
    if (scale != 2 || B <= 0 || H < 13 || W < 17 || (D != 128 && D != 256 && D != 384)) return 0;
    const int32_t h = (H + 1) / 2, w = (W + 1) / 2;
    const int64_t inner = mh_sgm_ws_bytes_ex(B, h, w, D / 2, paths, median), npix2 = (int64_t)B * h * w;
    return inner ? sgm_align16(2 * npix2) + inner + sgm_align16(npix2 * 4) : 0;
}

extern "C" int mh_sgm_proxy_scaled(const void* left, const void* right, int32_t frames_u8, void* ws, float* proxy, int32_t B, int32_t H, int32_t W, int32_t D,
                                   int32_t p1, int32_t p2, int32_t uniq, int32_t lr_tol, int32_t paths, int32_t median, int32_t scale, void* stream) {
    const char* who = "mh_sgm_proxy_scaled";
    MH_REQUIRE(scale == 1 || scale == 2, MH_ERR_ARG, "%s: scale must be 1 or 2", who);
    MH_REQUIRE(B > 0 && H > 0 && W > 0, MH_ERR_ARG, "%s: bad dimension", who);
    if (scale == 1) {
        MH_REQUIRE(D == 64 || D == 128 || D == 192, MH_ERR_ARG, "%s: at scale 1 D must be 64, 128 or 192", who);
        return sgm_proxy_impl(who, left, right, frames_u8, ws, proxy, B, H, W, D, p1, p2, uniq, lr_tol, paths, median, stream);
    }
    MH_REQUIRE(D == 128 || D == 256 || D == 384, MH_ERR_ARG, "%s: at scale 2 D is the full-resolution range and must be 128, 256 or 384", who);
    MH_REQUIRE(H >= 13 && W >= 17, MH_ERR_ARG, "%s: at scale 2 the half frame must hold one census window (H >= 13, W >= 17)", who);
    MH_REQUIRE(H <= 4 * 65535, MH_ERR_UNSUPPORTED, "%s: too many rows", who);
    const int32_t h = (H + 1) / 2, w = (W + 1) / 2;
    if (int e = sgm_check(who, left, right, ws, proxy, B, h, w, D / 2, p1, p2, uniq, lr_tol, paths, median)) return e;
    const int64_t npix2 = (int64_t)B * h * w;
    unsigned char* g2 = (unsigned char*)ws;                            // [2][B][h][w]
    unsigned char* inner = g2 + sgm_align16(2 * npix2);               // the matcher's own workspace on the half frame
    float* half = (float*)(inner + mh_sgm_ws_bytes_ex(B, h, w, D / 2, paths, median));      // the half-resolution labels [B][h][w]
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(sgm_half_gray_kernel, dim3((unsigned)mh_cdiv((int64_t)h * w, 256), (unsigned)(2 * B)), dim3(256), 0, s, left, right, g2, B, H, W, h, w, frames_u8 ? 1 : 0);
    if (int e = mh_check_launch("sgm_half_gray")) return e;
    if (int e = sgm_run(g2, g2 + npix2, 1, true, inner, half, B, h, w, D / 2, p1, p2, uniq, lr_tol, paths, median, stream)) return e;
    hipLaunchKernelGGL(sgm_upsample2_kernel, dim3((unsigned)mh_cdiv(W / 4 + 2, 64), (unsigned)mh_cdiv(H, 4), (unsigned)B), dim3(256), 0, s, (const float*)half, proxy, H, W, h, w);
    return mh_check_launch("sgm_upsample2");
}

// ---- speckle filter of a finished label map (mh_sgm_speckle): 4-connected components of the valid labels, the small ones set to 0 ------------------------------------
// Four launches, each reading only what an EARLIER launch (or itself, through atomics) wrote -- a kernel boundary is the one free coherence point between workgroups:
//   1. sgm_speckle_tile_kernel: components of one 64 x 16 tile by union-find in LDS; parent[p] = the tile-local root (the lowest pixel of the piece, itself for a root,
//      -1 for an invalid pixel), cnt[p] = the piece's pixel count at its root, 0 elsewhere.
//   2. sgm_speckle_merge_kernel: one thread per pixel pair across a tile border; joins the two roots.  Every access to `parent` in this launch is an integer atomic,
//      which executes at the memory side: no decision is taken on a cached word.
//   3. sgm_speckle_count_kernel: every tile-local root that is no longer a root adds its count to its final root (integer atomicAdd: associative, so the order of
//      arrival cannot change the sum) and leaves -(root + 1) in its own cnt.
//   4. sgm_speckle_apply_kernel: out = the label where its component's count exceeds max_size, else 0.
// Invariant of `parent` from launch 1 on: parent[p] <= p, parent[p] lies in p's component, and a word only ever decreases (atomicMin).  A walk up the parents
// therefore strictly decreases until it meets a root, whatever the other threads do meanwhile.  The final root of a component is its lowest pixel, the counts are
// integer sums: the result is a function of the input alone.
// ws: parent [B][H][W] (int32) | cnt [B][H][W] (int32), each rounded up to 16 bytes.  Every word is written by launch 1 before anything reads it.
#define SGM_ST_W 64
#define SGM_ST_H 16
#define SGM_ST_N (SGM_ST_W * SGM_ST_H)

#ifndef __HIPCC__
// the CPU emulator's header has atomicAdd only; its workgroups run on several OS threads
static inline int atomicMin(int* addr, int v) {
    int old = __atomic_load_n(addr, __ATOMIC_RELAXED);
    while (old > v && !__atomic_compare_exchange_n(addr, &old, v, false, __ATOMIC_RELAXED, __ATOMIC_RELAXED)) {}
    return old;
}
#endif

struct SpeckleArgs {
    const float* in; float* out;         // may be the same map: not __restrict__
    int* parent; int* cnt;
    int B, H, W, npix, max_size, nvb, nhb;      // nvb, nhb: tile borders inside a frame, between columns and between rows
    float max_diff;
};

__device__ __forceinline__ bool sgm_speckle_joined(float a, float b, float max_diff) { return a > 0.f && b > 0.f && fabsf(a - b) <= max_diff; }

// Union-find over the tile's pixels in LDS.  lab[i] <= i, only ever lowered by atomicMin, always to a pixel of i's own component.
// find: each step moves to a strictly lower index, so it ends; the word it read may have been lowered since, which makes the node it returns a non-root
// ancestor at worst -- unite does not trust it: the atomicMin's own return value says whether the node was still a root.
__device__ __forceinline__ int sgm_speckle_find_lds(int* lab, int x) {
    for (;;) { const int p = __atomic_load_n(lab + x, __ATOMIC_RELAXED); if (p == x) return x; x = p; }      // (atomic: a fresh ds_read per step, never a register copy)
}
// unite: joins the larger of the two found nodes to the smaller.  old == a: a was a root and now hangs under b, done.  Otherwise a had a parent `old` < a already:
// lab[a] is now min(old, b), still inside the component, and what remains to be joined is (old, b).  max(a, b) strictly decreases per round: it ends.
__device__ __forceinline__ void sgm_speckle_unite_lds(int* lab, int a, int b) {
    for (;;) {
        a = sgm_speckle_find_lds(lab, a); b = sgm_speckle_find_lds(lab, b);
        if (a == b) return;
        if (a < b) { const int t = a; a = b; b = t; }
        const int old = atomicMin(lab + a, b);
        if (old == a) return;
        a = old;
    }
}

// launch 1: grid (tiles x, tiles y, B), 256 threads, four pixels each (i = thread + 256 k: a wave covers one tile row)
__global__ __launch_bounds__(256) void sgm_speckle_tile_kernel(SpeckleArgs a) {
    __shared__ float s_v[SGM_ST_N];
    __shared__ int s_lab[SGM_ST_N];
    __shared__ int s_cnt[SGM_ST_N];
    const int x0 = (int)blockIdx.x * SGM_ST_W, y0 = (int)blockIdx.y * SGM_ST_H;
    const int frame = (int)blockIdx.z * a.H * a.W;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int i = (int)threadIdx.x + 256 * k, x = x0 + (i & (SGM_ST_W - 1)), y = y0 + i / SGM_ST_W;
        float v = 0.f;
        if (x < a.W && y < a.H) v = a.in[frame + y * a.W + x];
        s_v[i] = v > 0.f ? v : 0.f;                                     // NaN, 0, negative and outside the frame: 0 = joins nothing
        s_lab[i] = i; s_cnt[i] = 0;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int i = (int)threadIdx.x + 256 * k;
        const float v = s_v[i];
        if ((i & (SGM_ST_W - 1)) < SGM_ST_W - 1 && sgm_speckle_joined(v, s_v[i + 1], a.max_diff)) sgm_speckle_unite_lds(s_lab, i, i + 1);
        if (i < SGM_ST_N - SGM_ST_W && sgm_speckle_joined(v, s_v[i + SGM_ST_W], a.max_diff)) sgm_speckle_unite_lds(s_lab, i, i + SGM_ST_W);
    }
    __syncthreads();                                                    // s_lab is read-only from here: every find below returns the true root
    int root[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int i = (int)threadIdx.x + 256 * k;
        root[k] = s_v[i] > 0.f ? sgm_speckle_find_lds(s_lab, i) : -1;
        if (root[k] >= 0) atomicAdd(s_cnt + root[k], 1);
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int i = (int)threadIdx.x + 256 * k, x = x0 + (i & (SGM_ST_W - 1)), y = y0 + i / SGM_ST_W;
        if (x >= a.W || y >= a.H) continue;
        const int g = frame + y * a.W + x, r = root[k];
        a.parent[g] = r < 0 ? -1 : frame + (y0 + r / SGM_ST_W) * a.W + x0 + (r & (SGM_ST_W - 1));
        a.cnt[g] = r == i ? s_cnt[i] : 0;
    }
}

// The same union-find on the global `parent`, between workgroups of one launch.  A read is atomicMin(parent + x, x): parent[x] <= x makes it change nothing, and
// as a read-modify-write it is answered by the memory side with the word's present value, never by this CU's L1 or a register.  Termination as in LDS; the
// decisions (p == x, old == a) are taken on values the atomics returned.
__device__ __forceinline__ int sgm_speckle_find_atomic(int* parent, int x) {
    for (;;) { const int p = atomicMin(parent + x, x); if (p == x) return x; x = p; }
}

// the tile-local root of pixel x as launch 1 left it, from words this launch never writes: cnt (launch 3 writes it next) and the parent of a pixel that is no
// tile-local root (only roots are ever linked)
__device__ __forceinline__ int sgm_speckle_local_root(const SpeckleArgs& a, int x) { return a.cnt[x] > 0 ? x : a.parent[x]; }

// launch 2: one thread per pixel pair across a tile border, grid (pairs / 256, B): first the nvb column borders (H pairs each), then the nhb row borders (W pairs each).
// Neighbouring pairs of one border mostly join the same two tile-local pieces, and a large component would send every one of them up to the same root word: a pair
// whose predecessor along the border is joined too and has the same two tile-local roots leaves the work to it (by induction the first pair of such a run does it).
__global__ __launch_bounds__(256) void sgm_speckle_merge_kernel(SpeckleArgs a) {
    int e = (int)blockIdx.x * 256 + (int)threadIdx.x;
    const int frame = (int)blockIdx.y * a.H * a.W;
    int p, q, back;                                                     // back: the distance to the predecessor pair, 0 = none
    if (e < a.nvb * a.H) { const int bx = e / a.H, y = e - bx * a.H; q = frame + y * a.W + (bx + 1) * SGM_ST_W; p = q - 1; back = y ? a.W : 0; }
    else {
        e -= a.nvb * a.H;
        if (e >= a.nhb * a.W) return;
        const int by = e / a.W, x = e - by * a.W;
        q = frame + (by + 1) * SGM_ST_H * a.W + x; p = q - a.W; back = x ? 1 : 0;
    }
    if (!sgm_speckle_joined(a.in[p], a.in[q], a.max_diff)) return;
    const int pp = p - back, pq = q - back;
    p = sgm_speckle_local_root(a, p); q = sgm_speckle_local_root(a, q);
    if (back && sgm_speckle_joined(a.in[pp], a.in[pq], a.max_diff) && sgm_speckle_local_root(a, pp) == p && sgm_speckle_local_root(a, pq) == q) return;
    for (;;) {
        p = sgm_speckle_find_atomic(a.parent, p); q = sgm_speckle_find_atomic(a.parent, q);
        if (p == q) return;
        if (p < q) { const int t = p; p = q; q = t; }
        const int old = atomicMin(a.parent + p, q);
        if (old == p) return;
        p = old;
    }
}

// launches 3 and 4 only read `parent`: the walk ends at the component's root
__device__ __forceinline__ int sgm_speckle_find(const int* __restrict__ parent, int x) {
    for (;;) { const int p = parent[x]; if (p == x) return x; x = p; }
}

// launch 3: one thread per pixel.  c > 0 marks a tile-local root.  One that is not its component's root is never the target of an add (adds go to roots only), so the
// c it read is exact, and its cnt word is its own to overwrite.  A root may read its own count while adds arrive; any value it can see is > 0 and it does nothing.
__global__ __launch_bounds__(256) void sgm_speckle_count_kernel(SpeckleArgs a) {
    const int p = (int)blockIdx.x * 256 + (int)threadIdx.x;
    if (p >= a.npix) return;
    const int c = a.cnt[p];
    if (c <= 0) return;
    const int r = sgm_speckle_find(a.parent, p);
    if (r == p) return;
    atomicAdd(a.cnt + r, c);
    a.cnt[p] = -(r + 1);
}

// launch 4: one thread per pixel; every element of out is written.  A pixel that is no tile-local root (cnt 0) has its tile-local root as parent.
__global__ __launch_bounds__(256) void sgm_speckle_apply_kernel(SpeckleArgs a) {
    const int p = (int)blockIdx.x * 256 + (int)threadIdx.x;
    if (p >= a.npix) return;
    const float v = a.in[p];
    float o = 0.f;
    if (v > 0.f) {
        int n = a.cnt[p];
        if (n == 0) n = a.cnt[a.parent[p]];
        if (n < 0) n = a.cnt[-n - 1];
        if (n > a.max_size) o = v;
    }
    a.out[p] = o;
}

extern "C" int64_t mh_sgm_speckle_ws_bytes(int32_t B, int32_t H, int32_t W) {
    if (B <= 0 || H <= 0 || W <= 0) return 0;
    return 2 * sgm_align16((int64_t)B * H * W * 4);
}

extern "C" int mh_sgm_speckle(const float* labels, float* out, void* ws, int32_t B, int32_t H, int32_t W, int32_t max_size, float max_diff, void* stream) {
    MH_REQUIRE(labels && out && ws, MH_ERR_ARG, "mh_sgm_speckle: null argument");
    MH_REQUIRE(B > 0 && H > 0 && W > 0, MH_ERR_ARG, "mh_sgm_speckle: bad dimension");
    MH_REQUIRE(max_size >= 0, MH_ERR_ARG, "mh_sgm_speckle: max_size must not be negative");
    MH_REQUIRE(max_diff >= 0.f && max_diff < __builtin_inff(), MH_ERR_ARG, "mh_sgm_speckle: max_diff must be finite and not negative");
    MH_REQUIRE(mh_aligned16(ws), MH_ERR_ALIGN, "mh_sgm_speckle: ws must be 16-byte aligned");
    MH_REQUIRE((int64_t)B * H * W < (1ll << 31) - 256 && B < 65536 && H < 65536 * SGM_ST_H, MH_ERR_UNSUPPORTED, "mh_sgm_speckle: too many pixels or frames");
    const int64_t npix = (int64_t)B * H * W;
    SpeckleArgs a{};
    a.in = labels; a.out = out;
    a.parent = (int*)ws; a.cnt = (int*)((char*)ws + sgm_align16(npix * 4));
    a.B = B; a.H = H; a.W = W; a.npix = (int)npix; a.max_size = max_size; a.max_diff = max_diff;
    a.nvb = (W - 1) / SGM_ST_W; a.nhb = (H - 1) / SGM_ST_H;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(sgm_speckle_tile_kernel, dim3((unsigned)mh_cdiv(W, SGM_ST_W), (unsigned)mh_cdiv(H, SGM_ST_H), (unsigned)B), dim3(256), 0, s, a);
    if (int e = mh_check_launch("sgm_speckle_tile")) return e;
    const int64_t pairs = (int64_t)a.nvb * H + (int64_t)a.nhb * W;     // < 2 H W / 16
    if (pairs > 0) {
        hipLaunchKernelGGL(sgm_speckle_merge_kernel, dim3((unsigned)mh_cdiv(pairs, 256), (unsigned)B), dim3(256), 0, s, a);
        if (int e = mh_check_launch("sgm_speckle_merge")) return e;
        hipLaunchKernelGGL(sgm_speckle_count_kernel, dim3((unsigned)mh_cdiv(npix, 256)), dim3(256), 0, s, a);
        if (int e = mh_check_launch("sgm_speckle_count")) return e;
    }
    hipLaunchKernelGGL(sgm_speckle_apply_kernel, dim3((unsigned)mh_cdiv(npix, 256)), dim3(256), 0, s, a);
    mh_note_kernel("sgm_speckle_tile_kernel grid %d x %d x %d, %d launches", mh_cdiv(W, SGM_ST_W), mh_cdiv(H, SGM_ST_H), B, pairs > 0 ? 4 : 2);
    return mh_check_launch("sgm_speckle_apply");
}

// ---- preprocessing.colorize_img + the uint8 normalisation of TF's image summary (mh_colorize; the definition is the header's) -------------------------------------
// A few MB at the workload's size and launch-bound: a lane owns 4 consecutive pixels (one float4 in; 3 float4 or 3 dwords out), the colour map sits in LDS, and
// the two reductions (range over the batch, image_max over image 0) are per-workgroup partials that EVERY workgroup of the next launch finishes, as
// frame_apply_kernel finishes frame_sums_kernel's.  min / max are exact in any order, so capped grid-stride grids change no bit.
#include "colorize_lut.h"
#define CZ_MAX_PARTS 1024       // partials per reduction = workgroups of the launch that writes them
#define CZ_BAD 256              // the code of a non-finite pixel

struct ColorizeArgs {
    const float* value; void* out; float* mm; float* imax; unsigned short* code;
    int64_t n;                  // B * H * W
    int npix0, nmm, nimax;      // H * W; partial counts
    int cmap, use_range;
    float vmin, vmax;
};

static inline int colorize_parts(int64_t n) { const int64_t w = (n + 1023) / 1024; return (int)(w < CZ_MAX_PARTS ? w : CZ_MAX_PARTS); }

__device__ __forceinline__ bool colorize_finite(float v) { return fabsf(v) <= 3.402823466e+38f; }

// min and max over the workgroup (256 lanes): wave shuffles, then one LDS slot per wave.  Every lane takes part and every lane gets the result.
__device__ __forceinline__ void colorize_block_minmax(float& lo, float& hi, float (*red)[4]) {
    for (int o = 32; o > 0; o >>= 1) { lo = fminf(lo, __shfl_xor(lo, o)); hi = fmaxf(hi, __shfl_xor(hi, o)); }
    __syncthreads();                                    // (red may still be read from an earlier reduction)
    if ((threadIdx.x & 63) == 0) { red[0][threadIdx.x >> 6] = lo; red[1][threadIdx.x >> 6] = hi; }
    __syncthreads();
    lo = fminf(fminf(red[0][0], red[0][1]), fminf(red[0][2], red[0][3]));
    hi = fmaxf(fmaxf(red[1][0], red[1][1]), fmaxf(red[1][2], red[1][3]));
}

// four consecutive elements from q0 (q0 % 4 == 0, q0 < n); past the end: NaN, which no reduction counts and no store writes
__device__ __forceinline__ void colorize_load4(const float* __restrict__ value, int64_t q0, int64_t n, float (&v)[4]) {
    const float* p = value + q0;
    if (q0 + 4 <= n && (((uintptr_t)p) & 15u) == 0) {
        const float4 w = *reinterpret_cast<const float4*>(p);
        v[0] = w.x; v[1] = w.y; v[2] = w.z; v[3] = w.w;
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = q0 + j < n ? p[j] : __builtin_nanf("");
    }
}

// the colour map of this call in LDS: [256][3]
__device__ __forceinline__ void colorize_fill_lut(float* lut, int cmap) {
    for (int i = threadIdx.x; i < 768; i += 256) lut[i] = cmap ? MH_COLORIZE_JET[i / 3][i % 3] : (float)(i / 3) / 255.0f;
}

// step 1's range: the arguments, or the partial (min, max) pairs of colorize_minmax_kernel finished here
__device__ __forceinline__ void colorize_range(const ColorizeArgs& a, float (*red)[4], float& vmin, float& vmax) {
    if (a.use_range) { vmin = a.vmin; vmax = a.vmax; return; }
    float lo = __builtin_inff(), hi = -__builtin_inff();
    for (int i = threadIdx.x; i < a.nmm; i += 256) { lo = fminf(lo, a.mm[2 * i]); hi = fmaxf(hi, a.mm[2 * i + 1]); }
    colorize_block_minmax(lo, hi, red);
    vmin = lo; vmax = hi;
}

// idx of one value, or CZ_BAD
__device__ __forceinline__ int colorize_code(float v, float vmin, float den, bool flat) {
    MH_FP_EXACT
    if (!colorize_finite(v)) return CZ_BAD;
    if (flat) return 0;
    const float n = (v - vmin) / den;
    const float t = rintf(n * 255.0f);
    return t >= 255.0f ? 255 : (t > 0.0f ? (int)t : 0);
}

// launch 1 (use_range == 0): workgroup i writes the (min, max) of the finite elements of its quads, (+Inf, -Inf) when it saw none
__global__ __launch_bounds__(256) void colorize_minmax_kernel(ColorizeArgs a) {
    __shared__ float red[2][4];
    float lo = __builtin_inff(), hi = -__builtin_inff();
    const int64_t nquad = (a.n + 3) >> 2;
    for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < nquad; q += (int64_t)gridDim.x * 256) {
        float v[4];
        colorize_load4(a.value, q * 4, a.n, v);
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (colorize_finite(v[j])) { lo = fminf(lo, v[j]); hi = fmaxf(hi, v[j]); }
    }
    colorize_block_minmax(lo, hi, red);
    if (threadIdx.x == 0) { a.mm[2 * blockIdx.x] = lo; a.mm[2 * blockIdx.x + 1] = hi; }
}

// out_kind 0: range, index, table read; a lane writes its 4 pixels as 3 float4
__global__ __launch_bounds__(256) void colorize_float_kernel(ColorizeArgs a) {
    __shared__ float red[2][4];
    __shared__ float lut[768];
    colorize_fill_lut(lut, a.cmap);
    float vmin, vmax;
    colorize_range(a, red, vmin, vmax);
    __syncthreads();
    const float den = vmax - vmin;
    const bool flat = vmax == vmin;
    const int64_t q0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4;
    if (q0 >= a.n) return;
    float v[4], c[12];
    colorize_load4(a.value, q0, a.n, v);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int k = colorize_code(v[j], vmin, den, flat);
        const bool bad = k == CZ_BAD;
        const float* e = lut + 3 * (bad ? 0 : k);
        c[3 * j] = bad ? 1.0f : e[0]; c[3 * j + 1] = bad ? 0.0f : e[1]; c[3 * j + 2] = bad ? 0.0f : e[2];
    }
    float* dst = (float*)a.out + q0 * 3;
    if (q0 + 4 <= a.n && (((uintptr_t)dst) & 15u) == 0) {
#pragma unroll
        for (int k = 0; k < 3; ++k) reinterpret_cast<float4*>(dst)[k] = make_float4(c[4 * k], c[4 * k + 1], c[4 * k + 2], c[4 * k + 3]);
    } else {
#pragma unroll
        for (int k = 0; k < 12; ++k) if (q0 + k / 3 < a.n) dst[k] = c[k];
    }
}

// out_kind 1, first half: the codes of image 0 and, per workgroup, the largest channel of LUT[idx] over its pixels that are not bad (0 when it has none)
__global__ __launch_bounds__(256) void colorize_index_kernel(ColorizeArgs a) {
    __shared__ float red[2][4];
    __shared__ float lut[768];
    colorize_fill_lut(lut, a.cmap);
    float vmin, vmax;
    colorize_range(a, red, vmin, vmax);
    __syncthreads();
    const float den = vmax - vmin;
    const bool flat = vmax == vmin;
    float lo = 0.0f, hi = 0.0f;
    const int nquad = (a.npix0 + 3) >> 2;
    for (int q = (int)blockIdx.x * 256 + (int)threadIdx.x; q < nquad; q += (int)gridDim.x * 256) {
        float v[4];
        colorize_load4(a.value, (int64_t)q * 4, a.npix0, v);
        unsigned k[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            k[j] = (unsigned)colorize_code(v[j], vmin, den, flat);
            if (k[j] != CZ_BAD && q * 4 + j < a.npix0) hi = fmaxf(hi, fmaxf(fmaxf(lut[3 * k[j]], lut[3 * k[j] + 1]), lut[3 * k[j] + 2]));
        }
        unsigned short* dst = a.code + (int64_t)q * 4;                 // the code part starts 16-byte aligned: 8-byte aligned here
        if (q * 4 + 4 <= a.npix0) {
            *reinterpret_cast<uint2*>(dst) = make_uint2(k[0] | (k[1] << 16), k[2] | (k[3] << 16));
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) if (q * 4 + j < a.npix0) dst[j] = (unsigned short)k[j];
        }
    }
    colorize_block_minmax(lo, hi, red);
    if (threadIdx.x == 0) a.imax[blockIdx.x] = hi;
}

// out_kind 1, second half: image_max from the partials, then LUT[idx] * scale truncated to a byte.  Image 0 is a flat byte array: a lane's 4 pixels are 12 bytes =
// three dword stores; the last H * W % 4 pixels (and everything, when out is not 4-byte aligned) go out bytewise.
__global__ __launch_bounds__(256) void colorize_apply_kernel(ColorizeArgs a) {
    MH_FP_EXACT
    __shared__ float red[2][4];
    __shared__ float lut[768];
    colorize_fill_lut(lut, a.cmap);
    float lo = 0.0f, hi = 0.0f;
    for (int i = threadIdx.x; i < a.nimax; i += 256) hi = fmaxf(hi, a.imax[i]);
    colorize_block_minmax(lo, hi, red);                 // (its barriers also publish lut)
    const float scale = hi < 1e-6f ? 0.0f : 255.0f / hi;
    const int p0 = ((int)blockIdx.x * 256 + (int)threadIdx.x) * 4;
    if (p0 >= a.npix0) return;
    const bool full = p0 + 4 <= a.npix0;
    unsigned k[4] = {0u, 0u, 0u, 0u};
    if (full) {
        const uint2 w = *reinterpret_cast<const uint2*>(a.code + p0);
        k[0] = w.x & 0xffffu; k[1] = w.x >> 16; k[2] = w.y & 0xffffu; k[3] = w.y >> 16;
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) if (p0 + j < a.npix0) k[j] = a.code[p0 + j];
    }
    unsigned b[12];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const bool bad = k[j] == CZ_BAD;
        const float* e = lut + 3 * (bad ? 0u : k[j]);
        b[3 * j] = bad ? 255u : (unsigned)(e[0] * scale); b[3 * j + 1] = bad ? 0u : (unsigned)(e[1] * scale); b[3 * j + 2] = bad ? 0u : (unsigned)(e[2] * scale);
    }
    unsigned char* dst = (unsigned char*)a.out + (int64_t)p0 * 3;
    if (full && (((uintptr_t)dst) & 3u) == 0) {
#pragma unroll
        for (int w = 0; w < 3; ++w)
            reinterpret_cast<unsigned*>(dst)[w] = (b[4 * w] & 0xffu) | ((b[4 * w + 1] & 0xffu) << 8) | ((b[4 * w + 2] & 0xffu) << 16) | (b[4 * w + 3] << 24);
    } else {
#pragma unroll
        for (int i = 0; i < 12; ++i) if (p0 + i / 3 < a.npix0) dst[i] = (unsigned char)b[i];
    }
}

extern "C" int64_t mh_colorize_ws_bytes(int32_t B, int32_t H, int32_t W) {
    if (B <= 0 || H <= 0 || W <= 0) return 0;
    const int64_t npix0 = (int64_t)H * W;
    return sgm_align16((int64_t)colorize_parts(B * npix0) * 8) + sgm_align16((int64_t)colorize_parts(npix0) * 4) + sgm_align16(npix0 * 2);
}

extern "C" int mh_colorize(const float* value, void* out, void* ws, int32_t B, int32_t H, int32_t W, int32_t cmap, int32_t out_kind, int32_t use_range,
                           float vmin, float vmax, void* stream) {
    MH_REQUIRE(value && out && ws, MH_ERR_ARG, "mh_colorize: null argument");
    MH_REQUIRE(B > 0 && H > 0 && W > 0, MH_ERR_ARG, "mh_colorize: bad dimension");
    MH_REQUIRE(cmap == 0 || cmap == 1, MH_ERR_ARG, "mh_colorize: cmap must be 0 (gray) or 1 (jet)");
    MH_REQUIRE(out_kind == 0 || out_kind == 1, MH_ERR_ARG, "mh_colorize: out_kind must be 0 (float32 [B,H,W,3]) or 1 (uint8 [H,W,3] of image 0)");
    MH_REQUIRE(!use_range || (fabsf(vmin) < __builtin_inff() && fabsf(vmax) < __builtin_inff()), MH_ERR_ARG, "mh_colorize: vmin and vmax must be finite");
    MH_REQUIRE(mh_aligned16(ws), MH_ERR_ALIGN, "mh_colorize: ws must be 16-byte aligned");
    MH_REQUIRE((int64_t)B * H * W < (1ll << 31) - 1024, MH_ERR_UNSUPPORTED, "mh_colorize: too many pixels");
    ColorizeArgs a{};
    a.value = value; a.out = out;
    a.npix0 = H * W; a.n = (int64_t)B * a.npix0;
    a.nmm = colorize_parts(a.n); a.nimax = colorize_parts(a.npix0);
    a.mm = (float*)ws;
    a.imax = (float*)((char*)ws + sgm_align16((int64_t)a.nmm * 8));
    a.code = (unsigned short*)((char*)a.imax + sgm_align16((int64_t)a.nimax * 4));
    a.cmap = cmap; a.use_range = use_range ? 1 : 0; a.vmin = vmin; a.vmax = vmax;
    hipStream_t s = (hipStream_t)stream;
    if (!use_range) {
        hipLaunchKernelGGL(colorize_minmax_kernel, dim3((unsigned)a.nmm), dim3(256), 0, s, a);
        if (int e = mh_check_launch("colorize_minmax")) return e;
    }
    if (out_kind == 0) {
        hipLaunchKernelGGL(colorize_float_kernel, dim3((unsigned)mh_cdiv(a.n, 1024)), dim3(256), 0, s, a);
        mh_note_kernel("colorize_float_kernel grid %d, %d launch%s", mh_cdiv(a.n, 1024), use_range ? 1 : 2, use_range ? "" : "es");
        return mh_check_launch("colorize_float");
    }
    hipLaunchKernelGGL(colorize_index_kernel, dim3((unsigned)a.nimax), dim3(256), 0, s, a);
    if (int e = mh_check_launch("colorize_index")) return e;
    hipLaunchKernelGGL(colorize_apply_kernel, dim3((unsigned)mh_cdiv(a.npix0, 1024)), dim3(256), 0, s, a);
    mh_note_kernel("colorize_apply_kernel grid %d, %d launches", mh_cdiv(a.npix0, 1024), use_range ? 2 : 3);
    return mh_check_launch("colorize_apply");
}

extern "C" int mh_resize_image_fwd(const float* in, float* out, int32_t B, int32_t Hi, int32_t Wi, int32_t C, int32_t Ho, int32_t Wo,
                                   void* stream) {
    MH_REQUIRE(in && out && B > 0 && Hi > 0 && Wi > 0 && C > 0 && Ho > 0 && Wo > 0, MH_ERR_ARG, "mh_resize_image_fwd: bad argument");
    ResizeImgArgs a{in, nullptr, out, nullptr, B, Hi, Wi, C, Ho, Wo, (float)Hi / (float)Ho, (float)Wi / (float)Wo};
    hipLaunchKernelGGL(resize_image_fwd_kernel, dim3(grid_for((int64_t)B * Ho * Wo * C)), dim3(256), 0, (hipStream_t)stream, a);
    return mh_check_launch("resize_image_fwd");
}

extern "C" int mh_resize_image_bwd(const float* g, float* din, int32_t B, int32_t Hi, int32_t Wi, int32_t C, int32_t Ho, int32_t Wo,
                                   void* stream) {
    MH_REQUIRE(g && din && B > 0 && Hi > 0 && Wi > 0 && C > 0 && Ho > 0 && Wo > 0, MH_ERR_ARG, "mh_resize_image_bwd: bad argument");
    ResizeImgArgs a{nullptr, g, nullptr, din, B, Hi, Wi, C, Ho, Wo, (float)Hi / (float)Ho, (float)Wi / (float)Wo};
    hipLaunchKernelGGL(resize_image_bwd_kernel, dim3(grid_for((int64_t)B * Hi * Wi * C)), dim3(256), 0, (hipStream_t)stream, a);
    return mh_check_launch("resize_image_bwd");
}

extern "C" int mh_bilinear_sampler_fwd(const float* imgs, const float* coords, float* out, int32_t B, int32_t Hs, int32_t Ws, int32_t C,
                                       int32_t Ht, int32_t Wt, void* stream) {
    MH_REQUIRE(imgs && coords && out && B > 0 && Hs > 0 && Ws > 0 && C > 0 && Ht > 0 && Wt > 0, MH_ERR_ARG, "mh_bilinear_sampler_fwd: bad argument");
    MH_REQUIRE((int64_t)B * Hs * Ws < (1 << 24), MH_ERR_UNSUPPORTED,
               "mh_bilinear_sampler_fwd: B*Hs*Ws must stay below 2^24 (the reference computes the gather index in float32)");
    SamplerArgs a{imgs, coords, nullptr, out, nullptr, nullptr, B, Hs, Ws, C, Ht, Wt};
    hipLaunchKernelGGL(sampler_fwd_kernel, dim3(grid_for((int64_t)B * Ht * Wt)), dim3(256), 0, (hipStream_t)stream, a);
    return mh_check_launch("bilinear_sampler_fwd");
}

extern "C" int mh_bilinear_sampler_bwd(const float* g, const float* imgs, const float* coords, float* dcoords, float* dimgs, int32_t B,
                                       int32_t Hs, int32_t Ws, int32_t C, int32_t Ht, int32_t Wt, void* stream) {
    MH_REQUIRE(g && imgs && coords && (dcoords || dimgs) && B > 0 && Hs > 0 && Ws > 0 && C > 0 && Ht > 0 && Wt > 0, MH_ERR_ARG,
               "mh_bilinear_sampler_bwd: bad argument");
    MH_REQUIRE((int64_t)B * Hs * Ws < (1 << 24), MH_ERR_UNSUPPORTED, "mh_bilinear_sampler_bwd: B*Hs*Ws must stay below 2^24");
    SamplerArgs a{imgs, coords, g, nullptr, dcoords, dimgs, B, Hs, Ws, C, Ht, Wt};
    hipLaunchKernelGGL(sampler_bwd_kernel, dim3(grid_for((int64_t)B * Ht * Wt)), dim3(256), 0, (hipStream_t)stream, a);
    return mh_check_launch("bilinear_sampler_bwd");
}

extern "C" int mh_resize_bwd(const float* g, const float* in, float* din, int32_t accumulate, int32_t B, int32_t Hi, int32_t Wi,
                             int32_t Hr, int32_t Wr, int32_t cy, int32_t cx, int32_t Ho, int32_t Wo, float mul, int32_t mode,
                             void* stream) {
    MH_REQUIRE(g && in && din, MH_ERR_ARG, "mh_resize_bwd: null argument");
    ResizeArgs a{}; a.in = in; a.g = g; a.din = din; a.accumulate = accumulate;
    if (int e = resize_args(a, B, Hi, Wi, Hr, Wr, cy, cx, Ho, Wo, mul, mode)) return e;
    // rows of candidates per input pixel ~ 2 / sy (8 at an up-scaling of 4, 130 at 64: the full-resolution loss heads of the coarse
    // MAD blocks): split them over 4 / 16 / 64 lanes
    const int64_t npx = (int64_t)B * Hi * Wi;
    hipStream_t s = (hipStream_t)stream;
    if (a.sy <= 1.0f / 12.0f) hipLaunchKernelGGL((resize_bwd_kernel<64>), dim3(grid_for(npx * 64)), dim3(256), 0, s, a);
    else if (a.sy <= 1.0f / 6.0f) hipLaunchKernelGGL((resize_bwd_kernel<16>), dim3(grid_for(npx * 16)), dim3(256), 0, s, a);
    else if (a.sy <= 1.0f / 3.0f) hipLaunchKernelGGL((resize_bwd_kernel<4>), dim3(grid_for(npx * 4)), dim3(256), 0, s, a);
    else hipLaunchKernelGGL((resize_bwd_kernel<1>), dim3(grid_for(npx)), dim3(256), 0, s, a);
    return mh_check_launch("resize_bwd");
}

extern "C" int mh_head_bwd(const mh_head_bwd_desc* d, const float* src0, const float* src1, float* dV, void* dV_shadow, const float* w,
                           float* dx, const float* mask_ref, void* dx_shadow, void* stream) {
    MH_REQUIRE(d && dV && w && dx && (src0 || src1), MH_ERR_ARG, "mh_head_bwd: null argument");
    MH_REQUIRE(d->kind == 0 || d->kind == 1, MH_ERR_ARG, "mh_head_bwd: kind must be 0 (resize gradient of a finer level's du) or 1 (addends)");
    MH_REQUIRE(d->B > 0 && d->H > 0 && d->W > 0 && d->N >= 4 && d->N <= 64 && d->N % 4 == 0, MH_ERR_ARG, "mh_head_bwd: bad dimension (N = 4 .. 64, multiple of 4)");
    MH_REQUIRE(d->dx_ld % 4 == 0 && d->dx_ld >= d->N && mh_aligned16(dx) && mh_aligned16(w) && (!mask_ref || (d->mask_ld % 4 == 0 && mh_aligned16(mask_ref))) &&
               (!dx_shadow || mh_aligned16(dx_shadow)), MH_ERR_ALIGN, "mh_head_bwd: dx / mask / w must be 16-byte aligned with lds that are multiples of 4");
    HeadBwdArgs a{};
    if (d->kind == 0) {
        MH_REQUIRE(src0, MH_ERR_ARG, "mh_head_bwd: kind 0 needs the finer level's coordinate gradient");
        a.rz.g = src0;
        if (int e = resize_args(a.rz, d->B, d->H, d->W, d->Hr, d->Wr, d->cy, d->cx, d->Ho, d->Wo, d->mul, 0)) return e;
    } else {
        a.rz.B = d->B; a.rz.Hi = d->H; a.rz.Wi = d->W;
        a.a1 = src0; a.a2 = src1; a.a1_ld = d->src0_ld; a.a2_ld = d->src1_ld;
        MH_REQUIRE((!src0 || d->src0_ld >= 1) && (!src1 || d->src1_ld >= 1), MH_ERR_ARG, "mh_head_bwd: addend pixel strides must be >= 1");
    }
    a.dV = dV; a.dV_sh = (unsigned short*)dV_shadow; a.dV_sh_ld = 32;
    a.w = w; a.dx = dx; a.mask_ref = mask_ref; a.dx_sh = (unsigned short*)dx_shadow;
    a.N = d->N; a.dx_ld = d->dx_ld; a.mask_ld = d->mask_ld; a.dx_sh_ld = (d->N + 31) / 32 * 32; a.acc_dx = d->accumulate_dx; a.kind = d->kind;
    a.mask_alpha = d->mask_alpha;
    a.tiles_x = (d->W + HB_TW - 1) / HB_TW; a.tiles_y = (d->H + HB_TH - 1) / HB_TH;
    const int64_t grid = (int64_t)d->B * a.tiles_x * a.tiles_y;
    MH_REQUIRE(grid < (1ll << 31), MH_ERR_ARG, "mh_head_bwd: too many tiles");
    hipLaunchKernelGGL(head_bwd_kernel, dim3((unsigned)grid), dim3(256), 0, (hipStream_t)stream, a);
    mh_note_kernel("head_bwd_kernel kind %d N=%d", d->kind, d->N);
    return mh_check_launch("head_bwd");
}

extern "C" int mh_pad_reflect(const float* in, float* out, int32_t B, int32_t H, int32_t W, int32_t C,
                              int32_t Hp, int32_t Wp, int32_t pad_t, int32_t pad_l, int32_t out_ld,
                              float div, float sub, void* stream) {
    MH_REQUIRE(in && out, MH_ERR_ARG, "mh_pad_reflect: null argument");
    MH_REQUIRE(B > 0 && H > 1 && W > 1 && C > 0 && Hp >= H && Wp >= W && out_ld >= C, MH_ERR_ARG, "mh_pad_reflect: bad dimension");
    MH_REQUIRE(pad_t >= 0 && pad_l >= 0 && pad_t < H && pad_l < W && Hp - H - pad_t < H && Wp - W - pad_l < W &&
               Hp - H - pad_t >= 0 && Wp - W - pad_l >= 0, MH_ERR_ARG, "mh_pad_reflect: REFLECT pad must be smaller than the image");
    MH_REQUIRE(div != 0.f, MH_ERR_ARG, "mh_pad_reflect: div must be non-zero");
    PadArgs a{in, out, B, H, W, C, Hp, Wp, pad_t, pad_l, out_ld, div, sub};
    hipLaunchKernelGGL(pad_reflect_kernel, dim3(grid_for((int64_t)B * Hp * Wp)), dim3(256), 0, (hipStream_t)stream, a);
    return mh_check_launch("pad_reflect");
}

static inline int64_t nblk(int64_t n) { return (n + 255) / 256; }

// workgroups of loss_tile_kernel = partial sums per array: one LT_H x LT_W tile each, edge tiles included however few pixels they hold
static inline int64_t loss_tiles(int32_t B, int32_t H, int32_t W) { return (int64_t)B * mh_cdiv(W, LT_W) * mh_cdiv(H, LT_H); }

// [ maps: 8 n + 12 nw floats, unused since the tile kernel | L1 partial sums: one per tile | SSIM partial sums: one per tile ]
extern "C" int64_t mh_loss_ws_floats(int32_t B, int32_t H, int32_t W) {
    const int64_t n = (int64_t)B * H * W, nw = (int64_t)B * (H - 2) * (W - 2);
    return 8 * n + 12 * nw + 2 * loss_tiles(B, H, W);
}

extern "C" int mh_reprojection_loss(const float* left, const float* right, const float* disp, float* ws, float* result,
                                    float* ddisp, float grad_scale, int32_t B, int32_t H, int32_t W, void* stream) {
    return mh_reprojection_loss_phase(left, right, disp, ws, result, ddisp, grad_scale, B, H, W, 0, stream);
}

extern "C" int mh_reprojection_loss_phase(const float* left, const float* right, const float* disp, float* ws, float* result,
                                          float* ddisp, float grad_scale, int32_t B, int32_t H, int32_t W, int32_t phase, void* stream) {
    MH_REQUIRE(phase >= 0 && phase <= 2, MH_ERR_ARG, "mh_reprojection_loss_phase: phase must be 0 (all), 1 (maps + gradient) or 2 (final reduction)");
    MH_REQUIRE(left && right && disp && ws && result, MH_ERR_ARG, "mh_reprojection_loss: null argument");
    MH_REQUIRE(B > 0 && H >= 3 && W >= 3, MH_ERR_ARG, "mh_reprojection_loss: image must be at least 3x3");
    MH_REQUIRE(mh_aligned16(ws), MH_ERR_ALIGN, "mh_reprojection_loss: workspace must be 16-byte aligned");
    const int64_t n = (int64_t)B * H * W, nw = (int64_t)B * (H - 2) * (W - 2);
    MH_REQUIRE(n * 12 < (1ll << 31) - 64, MH_ERR_ARG, "mh_reprojection_loss: too many pixels (32-bit byte offsets into the frames)");
    LossArgs a{};
    a.left = left; a.right = right; a.disp = disp; a.result = result; a.ddisp = ddisp; a.grad_scale = grad_scale;
    a.B = B; a.H = H; a.W = W;
    const int tiles_x = mh_cdiv(W, LT_W), tiles_y = mh_cdiv(H, LT_H);
    const int64_t ntiles = loss_tiles(B, H, W);                           // the count mh_loss_ws_floats sizes the two partial arrays with
    MH_REQUIRE(ntiles < (1ll << 31), MH_ERR_ARG, "mh_reprojection_loss: too many tiles");
    a.rep = ws; a.drep = ws + 4 * n; a.coef = ws + 8 * n;                  // (maps: LDS only since the tile kernel; the offsets keep the layout)
    a.part1 = ws + 8 * n + 12 * nw; a.nblk1 = (int)ntiles;
    a.part2 = a.part1 + ntiles; a.nblk2 = (int)ntiles;
    hipStream_t s = (hipStream_t)stream;
    if (phase != 2) hipLaunchKernelGGL(loss_tile_kernel<false>, dim3((unsigned)ntiles), dim3(256), 0, s, a, tiles_x, tiles_y, ddisp ? 1 : 0, LossMask{});
    if (phase != 1) hipLaunchKernelGGL(loss_final_kernel<false>, dim3(1), dim3(256), 0, s, a, LossMask{});
    return mh_check_launch("reprojection_loss");
}

// The masks and the counts of the masked loss live in the retired map region of the loss workspace, behind the smoothness partial sums (one float per tile):
//   [ smoothness: T floats | pad to 4 floats | left mask: n bytes | pad to 16 bytes | right mask: n bytes | pad to 16 bytes | counts: 2 T ints | ... ]
// with n = B H W and T = loss_tiles <= n.  In floats: at most (T + 3) + 2 (n / 4 + 4) + 2 T <= 3.5 n + 11 <= 8 n for every n >= 9 (H, W >= 3).
static inline int64_t loss_mask_floats(int64_t n) { return (n + 15) / 16 * 4; }
extern "C" int64_t mh_loss_valid_offset(int32_t B, int32_t H, int32_t W) { return (loss_tiles(B, H, W) + 3) / 4 * 4; }

extern "C" int mh_reprojection_loss_masked(const float* left, const float* right, const float* disp, const uint8_t* valid_l, const uint8_t* valid_r, float* ws,
                                           float* result, float* ddisp, float grad_scale, int32_t B, int32_t H, int32_t W, int32_t phase, void* stream) {
    MH_REQUIRE(phase >= 0 && phase <= 2, MH_ERR_ARG, "mh_reprojection_loss_masked: phase must be 0 (all), 1 (counts + maps + gradient) or 2 (final reduction)");
    MH_REQUIRE(left && right && disp && ws && result, MH_ERR_ARG, "mh_reprojection_loss_masked: null argument");
    MH_REQUIRE(valid_l && valid_r, MH_ERR_ARG, "mh_reprojection_loss_masked: null validity mask");
    MH_REQUIRE(B > 0 && H >= 3 && W >= 3, MH_ERR_ARG, "mh_reprojection_loss_masked: image must be at least 3x3");
    MH_REQUIRE(mh_aligned16(ws), MH_ERR_ALIGN, "mh_reprojection_loss_masked: workspace must be 16-byte aligned");
    const int64_t n = (int64_t)B * H * W, nw = (int64_t)B * (H - 2) * (W - 2);
    MH_REQUIRE(n * 12 < (1ll << 31) - 64, MH_ERR_ARG, "mh_reprojection_loss_masked: too many pixels (32-bit byte offsets into the frames)");
    LossArgs a{};
    a.left = left; a.right = right; a.disp = disp; a.result = result; a.ddisp = ddisp; a.grad_scale = grad_scale;
    a.B = B; a.H = H; a.W = W;
    const int tiles_x = mh_cdiv(W, LT_W), tiles_y = mh_cdiv(H, LT_H);
    const int64_t ntiles = loss_tiles(B, H, W);
    a.part1 = ws + 8 * n + 12 * nw; a.nblk1 = (int)ntiles;
    a.part2 = a.part1 + ntiles; a.nblk2 = (int)ntiles;
    const int64_t cnt_off = mh_loss_valid_offset(B, H, W) + 2 * loss_mask_floats(n);
    MH_REQUIRE(cnt_off + 2 * ntiles <= 8 * n + 12 * nw, MH_ERR_ARG, "mh_reprojection_loss_masked: the counts do not fit in front of the partial sums");
    const LossMask m{valid_l, valid_r, (int*)(ws + cnt_off)};
    hipStream_t s = (hipStream_t)stream;
    if (phase != 2) {
        hipLaunchKernelGGL(loss_count_kernel, dim3((unsigned)ntiles), dim3(256), 0, s, a, tiles_x, tiles_y, m);
        hipLaunchKernelGGL(loss_tile_kernel<true>, dim3((unsigned)ntiles), dim3(256), 0, s, a, tiles_x, tiles_y, ddisp ? 1 : 0, m);
    }
    if (phase != 1) hipLaunchKernelGGL(loss_final_kernel<true>, dim3(1), dim3(256), 0, s, a, m);
    return mh_check_launch("reprojection_loss_masked");
}

// one partial sum per tile of smooth_tile_kernel: the tiling of the reprojection loss
extern "C" int64_t mh_smoothness_ws_floats(int32_t B, int32_t H, int32_t W) { return loss_tiles(B, H, W); }

extern "C" int mh_smoothness_loss(const float* disp, const float* image, float* ws, float* result, float* ddisp, float weight, float grad_scale,
                                  int32_t accumulate, int32_t B, int32_t H, int32_t W, int32_t C, int32_t phase, void* stream) {
    MH_REQUIRE(phase >= 0 && phase <= 2, MH_ERR_ARG, "mh_smoothness_loss: phase must be 0 (all), 1 (tiles: partial sums + gradient) or 2 (final reduction)");
    MH_REQUIRE(disp && image && ws && result, MH_ERR_ARG, "mh_smoothness_loss: null argument");
    MH_REQUIRE(B > 0 && H > 0 && W > 0, MH_ERR_ARG, "mh_smoothness_loss: bad dimension");
    MH_REQUIRE(C == 1 || C == 3, MH_ERR_ARG, "mh_smoothness_loss: the image has 1 or 3 channels");
    MH_REQUIRE((int64_t)B * H * W < (1ll << 31), MH_ERR_ARG, "mh_smoothness_loss: too many pixels");
    const int tiles_x = mh_cdiv(W, LT_W), tiles_y = mh_cdiv(H, LT_H);
    const int64_t ntiles = loss_tiles(B, H, W);
    MH_REQUIRE(ntiles < (1ll << 31), MH_ERR_ARG, "mh_smoothness_loss: too many tiles");
    SmoothArgs a{disp, image, ws, result, ddisp, B, H, W, C, (int)ntiles, accumulate ? 1 : 0, weight, grad_scale};
    hipStream_t s = (hipStream_t)stream;
    if (phase != 2) hipLaunchKernelGGL(smooth_tile_kernel, dim3((unsigned)ntiles), dim3(256), 0, s, a, tiles_x, tiles_y);
    if (phase != 1) hipLaunchKernelGGL(smooth_final_kernel, dim3(1), dim3(256), 0, s, a);
    return mh_check_launch("mh_smoothness_loss");
}

extern "C" int64_t mh_metrics_ws_floats(int32_t B, int32_t H, int32_t W) { return 3 * nblk((int64_t)B * H * W) + 16; }

extern "C" int mh_metrics(const float* disp, const float* gt, float* ws, float* result, float pixel_th,
                          int32_t B, int32_t H, int32_t W, void* stream) {
    MH_REQUIRE(disp && gt && ws && result, MH_ERR_ARG, "mh_metrics: null argument");
    MH_REQUIRE(B > 0 && H > 0 && W > 0, MH_ERR_ARG, "mh_metrics: bad dimension");
    MetArgs a{disp, gt, ws, result, (int64_t)B * H * W, (int)nblk((int64_t)B * H * W), pixel_th};
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(metrics_kernel, dim3(a.nblk), dim3(256), 0, s, a);
    hipLaunchKernelGGL(metrics_final_kernel, dim3(1), dim3(256), 0, s, a);
    return mh_check_launch("metrics");
}

extern "C" int64_t mh_proxy_ws_floats(int32_t B, int32_t H, int32_t W) { return 2 * nblk((int64_t)B * H * W); }

static int masked_l1(const char* what, const float* pred, const float* target, float* ws, float* result, float* dpred, float weight,
                     float grad_scale, float hi, int zero_only, int32_t B, int32_t H, int32_t W, void* stream) {
    MH_REQUIRE(pred && target && ws && result, MH_ERR_ARG, "%s: null argument", what);
    MH_REQUIRE(B > 0 && H > 0 && W > 0, MH_ERR_ARG, "%s: bad dimension", what);
    ProxyArgs a{pred, target, ws, result, dpred, (int64_t)B * H * W, (int)nblk((int64_t)B * H * W), weight, grad_scale, hi, zero_only, 0.f};
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL((proxy_partial_kernel<0, false>), dim3(a.nblk), dim3(256), 0, s, a);
    hipLaunchKernelGGL(proxy_final_kernel, dim3(1), dim3(256), 0, s, a);
    if (dpred) hipLaunchKernelGGL((proxy_grad_kernel<0>), dim3(a.nblk), dim3(256), 0, s, a);
    return mh_check_launch(what);
}

// the launches of mh_label_loss for one per-pixel term: a.norm > 0 = fixed normaliser, the gradient leaves with the partial sums
template <int FAM> static void label_loss_launch(const ProxyArgs& a, hipStream_t s) {
    const bool fused = a.norm > 0.f && a.dpred;
    if (fused) hipLaunchKernelGGL((proxy_partial_kernel<FAM, true>), dim3(a.nblk), dim3(256), 0, s, a);
    else hipLaunchKernelGGL((proxy_partial_kernel<FAM, false>), dim3(a.nblk), dim3(256), 0, s, a);
    hipLaunchKernelGGL(proxy_final_kernel, dim3(1), dim3(256), 0, s, a);
    if (a.dpred && !fused) hipLaunchKernelGGL((proxy_grad_kernel<FAM>), dim3(a.nblk), dim3(256), 0, s, a);
}

// normaliser of loss `loss` over npix pixels: 0 = sum(valid) (mean_l1, mean_l2), 1 (sum_*), npix (mean_huber)
static inline float label_loss_norm(int32_t loss, int64_t npix) {
    if (loss == MH_LOSS_MEAN_L1 || loss == MH_LOSS_MEAN_L2) return 0.f;
    return loss == MH_LOSS_MEAN_HUBER ? (float)npix : 1.0f;
}

extern "C" int mh_label_loss(const float* pred, const float* label, float* ws, float* result, float* dpred, int32_t loss, int32_t rule, float hi, float weight,
                             float grad_scale, int32_t B, int32_t H, int32_t W, void* stream) {
    MH_REQUIRE(pred && label && ws && result, MH_ERR_ARG, "mh_label_loss: null argument");
    MH_REQUIRE(loss >= MH_LOSS_MEAN_L1 && loss <= MH_LOSS_SUM_HUBER, MH_ERR_ARG, "mh_label_loss: loss must be one of MH_LOSS_* (0 .. 5)");
    MH_REQUIRE(rule == 0 || rule == 1, MH_ERR_ARG, "mh_label_loss: rule must be 0 (proxy) or 1 (supervised)");
    MH_REQUIRE(hi > 0.f, MH_ERR_ARG, "mh_label_loss: hi must be positive");
    MH_REQUIRE(B > 0 && H > 0 && W > 0, MH_ERR_ARG, "mh_label_loss: bad dimension");
    const int64_t npix = (int64_t)B * H * W;
    MH_REQUIRE(nblk(npix) < (1ll << 31), MH_ERR_ARG, "mh_label_loss: too many pixels");
    ProxyArgs a{pred, label, ws, result, dpred, npix, (int)nblk(npix), weight, grad_scale, hi, rule, label_loss_norm(loss, npix)};
    hipStream_t s = (hipStream_t)stream;
    switch (loss >> 1) {
        case 0: label_loss_launch<0>(a, s); break;
        case 1: label_loss_launch<1>(a, s); break;
        default: label_loss_launch<2>(a, s); break;
    }
    return mh_check_launch("mh_label_loss");
}

extern "C" int mh_proxy_loss(const float* pred, const float* proxy, float* ws, float* result, float* dpred, float weight,
                             float grad_scale, int32_t B, int32_t H, int32_t W, void* stream) {
    return masked_l1("mh_proxy_loss", pred, proxy, ws, result, dpred, weight, grad_scale, 192.0f, 0, B, H, W, stream);
}

extern "C" int mh_supervised_loss(const float* pred, const float* target, float* ws, float* result, float* dpred, float weight,
                                  float grad_scale, float max_disp, int32_t B, int32_t H, int32_t W, void* stream) {
    MH_REQUIRE(max_disp > 0.f, MH_ERR_ARG, "mh_supervised_loss: max_disp must be positive");
    return masked_l1("mh_supervised_loss", pred, target, ws, result, dpred, weight, grad_scale, max_disp, 1, B, H, W, stream);
}

extern "C" int64_t mh_proxy_scaled_ws_floats(int32_t B, int32_t H, int32_t W, int32_t scale) {
    if (scale < 1) scale = 1;
    return 2 * nblk((int64_t)B * (H / scale) * (W / scale));
}

template <int FAM> static void label_loss_scaled_launch(const ProxySArgs& a, const ProxyArgs& f, hipStream_t s) {
    const int ggrid = grid_for((int64_t)a.B * a.H * a.W);
    const bool fused = a.norm > 0.f && a.dpred;
    if (fused) hipLaunchKernelGGL((proxy_s_fused_kernel<FAM>), dim3(f.nblk > ggrid ? f.nblk : ggrid), dim3(256), 0, s, a, f.nblk);
    else hipLaunchKernelGGL((proxy_s_partial_kernel<FAM>), dim3(f.nblk), dim3(256), 0, s, a);
    hipLaunchKernelGGL(proxy_final_kernel, dim3(1), dim3(256), 0, s, f);
    if (a.dpred && !fused) hipLaunchKernelGGL((proxy_s_grad_kernel<FAM>), dim3(ggrid), dim3(256), 0, s, a);
}

static int label_loss_scaled(const char* what, const float* pred, const float* proxy, float* ws, float* result, float* dpred, int32_t loss, float weight,
                             float grad_scale, int32_t scale, int32_t B, int32_t H, int32_t W, void* stream) {
    MH_REQUIRE(pred && proxy && ws && result, MH_ERR_ARG, "%s: null argument", what);
    MH_REQUIRE(loss >= MH_LOSS_MEAN_L1 && loss <= MH_LOSS_SUM_HUBER, MH_ERR_ARG, "%s: loss must be one of MH_LOSS_* (0 .. 5)", what);
    MH_REQUIRE(B > 0 && H > 0 && W > 0 && H < 65536 && W < 65536, MH_ERR_ARG, "%s: bad dimension", what);
    MH_REQUIRE(scale >= 1 && scale <= H && scale <= W, MH_ERR_ARG, "%s: scale must lie in 1 .. min(H, W)", what);
    const int Hs = H / scale, Ws = W / scale;
    const int64_t nout = (int64_t)B * Hs * Ws;
    MH_REQUIRE((int64_t)B * H * W < (1ll << 31), MH_ERR_ARG, "%s: too many pixels", what);
    const float norm = label_loss_norm(loss, nout);
    ProxySArgs a{pred, proxy, ws, result, dpred, B, H, W, Hs, Ws, (float)H / (float)Hs, (float)W / (float)Ws, (float)scale, weight, grad_scale, norm};
    ProxyArgs f{};                                                     // (the final reduction is the un-scaled loss's)
    f.part = ws; f.result = result; f.nblk = (int)nblk(nout); f.weight = weight; f.norm = norm;
    hipStream_t s = (hipStream_t)stream;
    switch (loss >> 1) {
        case 0: label_loss_scaled_launch<0>(a, f, s); break;
        case 1: label_loss_scaled_launch<1>(a, f, s); break;
        default: label_loss_scaled_launch<2>(a, f, s); break;
    }
    return mh_check_launch(what);
}

extern "C" int mh_proxy_loss_scaled(const float* pred, const float* proxy, float* ws, float* result, float* dpred, float weight,
                                    float grad_scale, int32_t scale, int32_t B, int32_t H, int32_t W, void* stream) {
    return label_loss_scaled("mh_proxy_loss_scaled", pred, proxy, ws, result, dpred, MH_LOSS_MEAN_L1, weight, grad_scale, scale, B, H, W, stream);
}

extern "C" int mh_label_loss_scaled(const float* pred, const float* label, float* ws, float* result, float* dpred, int32_t loss, float weight,
                                    float grad_scale, int32_t scale, int32_t B, int32_t H, int32_t W, void* stream) {
    return label_loss_scaled("mh_label_loss_scaled", pred, label, ws, result, dpred, loss, weight, grad_scale, scale, B, H, W, stream);
}

extern "C" int64_t mh_metrics_kitti_ws_floats(int32_t B, int32_t H, int32_t W) { return 3 * nblk((int64_t)B * H * W) + 16; }

extern "C" int mh_metrics_kitti(const float* disp, const float* gt, float* ws, float* result, int32_t B, int32_t H, int32_t W, void* stream) {
    MH_REQUIRE(disp && gt && ws && result, MH_ERR_ARG, "mh_metrics_kitti: null argument");
    MH_REQUIRE(B > 0 && H > 0 && W > 0, MH_ERR_ARG, "mh_metrics_kitti: bad dimension");
    MH_REQUIRE((int64_t)B * H * W < (1ll << 31), MH_ERR_ARG, "mh_metrics_kitti: too many pixels");
    KittiArgs a{disp, gt, ws, result, (int64_t)B * H * W, (int)nblk((int64_t)B * H * W)};
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(metrics_kitti_kernel, dim3(a.nblk), dim3(256), 0, s, a);
    hipLaunchKernelGGL(metrics_kitti_final_kernel, dim3(1), dim3(256), 0, s, a);
    return mh_check_launch("mh_metrics_kitti");
}

extern "C" int mh_adam(float* var, float* m, float* v, const float* grad, int64_t n, const float* state, float lr, float beta1,
                       float beta2, float eps, float grad_scale, void* stream) {
    MH_REQUIRE(var && m && v && grad && state && n > 0, MH_ERR_ARG, "mh_adam: bad argument");
    MH_REQUIRE(beta1 >= 0.f && beta1 < 1.f && beta2 >= 0.f && beta2 < 1.f, MH_ERR_ARG, "mh_adam: beta out of [0, 1)");
    hipLaunchKernelGGL(adam_kernel, dim3(grid_for(n)), dim3(256), 0, (hipStream_t)stream, var, m, v, grad, n, state, lr, beta1, beta2, eps, grad_scale);
    return mh_check_launch("adam");
}

extern "C" int mh_adam_advance(float* state, float beta1, float beta2, void* stream) {
    MH_REQUIRE(state, MH_ERR_ARG, "mh_adam_advance: null state");
    hipLaunchKernelGGL(adam_advance_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, state, beta1, beta2);
    return mh_check_launch("adam_advance");
}

extern "C" int mh_momentum(float* var, float* accum, const float* grad, int64_t n, float lr, float momentum,
                           float grad_scale, void* stream) {
    MH_REQUIRE(var && accum && grad && n > 0, MH_ERR_ARG, "mh_momentum: bad argument");
    const int64_t n4 = n >> 2;
    if (n4 > 0 && (((uintptr_t)var | (uintptr_t)accum | (uintptr_t)grad) & 15u) == 0)
        hipLaunchKernelGGL(momentum4_kernel, dim3(grid_for(n4)), dim3(256), 0, (hipStream_t)stream, (float4*)var, (float4*)accum, (const float4*)grad, n4, lr, momentum,
                           grad_scale);
    else if (n4 > 0) { hipLaunchKernelGGL(momentum_kernel, dim3(grid_for(n)), dim3(256), 0, (hipStream_t)stream, var, accum, grad, n, lr, momentum, grad_scale); return mh_check_launch("momentum"); }
    if (n & 3)          // (the tail of a range that is not a multiple of 4)
        hipLaunchKernelGGL(momentum_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, var + 4 * n4, accum + 4 * n4, grad + 4 * n4, n & 3, lr, momentum, grad_scale);
    return mh_check_launch("momentum");
}

extern "C" int mh_copy_channels(const float* src, int32_t src_ld, float* dst, int32_t dst_ld, int64_t npix,
                                int32_t nch, float scale, int32_t accumulate, void* stream) {
    MH_REQUIRE(src && dst && npix > 0 && nch > 0 && src_ld >= nch && dst_ld >= nch, MH_ERR_ARG, "mh_copy_channels: bad argument");
    hipLaunchKernelGGL(copy_channels_kernel, dim3(grid_for(npix * nch)), dim3(256), 0, (hipStream_t)stream,
                       src, src_ld, dst, dst_ld, npix, nch, scale, accumulate);
    return mh_check_launch("copy_channels");
}

extern "C" int mh_leaky_bwd(float* dy, int32_t dy_ld, const float* y, int32_t y_ld, int64_t npix, int32_t nch,
                            float alpha, void* stream) {
    MH_REQUIRE(dy && y && npix > 0 && nch > 0, MH_ERR_ARG, "mh_leaky_bwd: bad argument");
    hipLaunchKernelGGL(leaky_bwd_kernel, dim3(grid_for(npix * nch)), dim3(256), 0, (hipStream_t)stream, dy, dy_ld, y, y_ld, npix, nch, alpha);
    return mh_check_launch("leaky_bwd");
}

extern "C" int mh_bias_grad(const float* dz, int32_t dz_ld, int64_t npix, int32_t nch, float* db, void* stream) {
    MH_REQUIRE(dz && db && npix > 0 && nch > 0 && dz_ld >= nch, MH_ERR_ARG, "mh_bias_grad: bad argument");
    int nchp = 1;
    while (nchp < nch && nchp < 64) nchp <<= 1;
    const int64_t rows = (npix + (64 / nchp) - 1) / (64 / nchp);          // wave rows of work
    int gx = (int)((rows + 4 * 8 - 1) / (4 * 8));                          // ~8 rows per wave
    if (gx > 1024) gx = 1024;
    if (gx < 1) gx = 1;
    hipLaunchKernelGGL(bias_grad_kernel, dim3(gx, (nch + 63) / 64), dim3(256), 0, (hipStream_t)stream, dz, dz_ld, npix, nch, db, nchp, (float*)nullptr);
    return mh_check_launch("bias_grad");
}

extern "C" int mh_bias_grad_blocks(int64_t npix, int32_t nch) {
    if (npix <= 0 || nch <= 0) return 0;
    int nchp = 1;
    while (nchp < nch && nchp < 64) nchp <<= 1;
    const int64_t rows = (npix + (64 / nchp) - 1) / (64 / nchp);
    int64_t gx = (rows + 4 * 8 - 1) / (4 * 8);
    return (int)(gx > 1024 ? 1024 : (gx < 1 ? 1 : gx));
}

extern "C" int mh_bias_grad_partial(const float* dz, int32_t dz_ld, int64_t npix, int32_t nch, float* ws, int32_t nblocks, void* stream) {
    MH_REQUIRE(dz && ws && npix > 0 && nch > 0 && dz_ld >= nch, MH_ERR_ARG, "mh_bias_grad_partial: bad argument");
    MH_REQUIRE(nblocks == mh_bias_grad_blocks(npix, nch), MH_ERR_ARG, "mh_bias_grad_partial: nblocks %d must be mh_bias_grad_blocks(npix, nch) = %d (the workspace was sized for it)",
               nblocks, mh_bias_grad_blocks(npix, nch));
    int nchp = 1;
    while (nchp < nch && nchp < 64) nchp <<= 1;
    hipLaunchKernelGGL(bias_grad_kernel, dim3(nblocks, (nch + 63) / 64), dim3(256), 0, (hipStream_t)stream, dz, dz_ld, npix, nch, (float*)nullptr, nchp, ws);
    return mh_check_launch("bias_grad_partial");
}

// device time stamp (diagnostics of the replayed step: where the side lane starts, how long the tail behind the last input gradient is):
// one lane stores the constant-rate wall clock (s_memrealtime, 100 MHz on gfx950) into a slot.  A plan op like any other, so the stamp sits at
// its place in the captured graph and needs no tracer (rocprofv3 shifts the side queue by ~0.3 ms: profiles/r03_experiments.txt #3).
// deterministic mode: float buffer += its fixed-point twin (value * 2^48), twin cleared (mh_common.h: mh_atomic_add)
__global__ __launch_bounds__(256) void det_flush_kernel(float* dst, long long* acc, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const long long a = acc[i];
        if (a) { dst[i] += (float)((double)a * (1.0 / 281474976710656.0)); acc[i] = 0; }
    }
}
extern "C" int mh_det_flush(float* dst, void* acc, int64_t n, void* stream) {
    MH_REQUIRE(dst && acc && n >= 0, MH_ERR_ARG, "mh_det_flush: null buffer");
    if (n == 0) return 0;
    const int64_t blocks = (n + 255) / 256;
    hipLaunchKernelGGL(det_flush_kernel, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(256), 0, (hipStream_t)stream, dst, (long long*)acc, n);
    return mh_check_launch("det_flush");
}

__global__ void stamp_kernel(long long* slot) { *slot = wall_clock64(); }
extern "C" int mh_stamp(void* slot, void* stream) {
    MH_REQUIRE(slot && (((uintptr_t)slot) & 7u) == 0, MH_ERR_ARG, "mh_stamp: 8-byte aligned slot");
    hipLaunchKernelGGL(stamp_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, (long long*)slot);
    return mh_check_launch("stamp");
}
extern "C" int64_t mh_stamp_rate_khz(void) {
    int dev = 0, khz = 0;
    if (hipGetDevice(&dev) != hipSuccess) return 0;
    if (hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, dev) != hipSuccess) return 0;
    return khz;
}

extern "C" int mh_fill(float* p, int64_t n, float v, void* stream) {
    MH_REQUIRE(p && n > 0, MH_ERR_ARG, "mh_fill: bad argument");
    hipLaunchKernelGGL(fill_kernel, dim3(grid_for(n)), dim3(256), 0, (hipStream_t)stream, p, n, v);
    return mh_check_launch("fill");
}

// this translation unit's copy of the deterministic-accumulation table (mh_common.h)
extern "C" int mh_det_sync_ops(const void* t) { return mh_det_upload(*reinterpret_cast<const mh_det_table*>(t)); }
extern "C" int mh_det_ovf_ops(void) { return mh_det_overflow_take(); }      // this translation unit's saturation flag of the deterministic twin (mh_common.h)
