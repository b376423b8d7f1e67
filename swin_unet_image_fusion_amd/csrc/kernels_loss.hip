// The reference's fusion loss (a008_loss.py MyLoss) for single-channel fp32 images, value and d total / d fusion.
//
// The operators are restated from the published definitions of the kornia classes the reference calls (MS_SSIMLoss, ssim_loss, Sobel,
// PSNRLoss); kornia is not available to this build, so PARITY WITH KORNIA ITSELF IS UNPINNED.  tests/loss_restatement.py
// is the same text in torch and is what these kernels are checked against.
//
// Kernels, all on one stream, no atomics, every sum in a fixed order:
//   loss_pointwise_kernel   Sobel texture, intensity and squared-error partial sums of a 32x32 tile; writes the texture + intensity
//                           gradient (adjoint of the replicate-border Sobel in gather form).
//   loss_moments_kernel     SSIM term.  A tile of fusion / ir / vis with its halo lives in LDS; per Gaussian scale a row pass and a
//                           column pass give the 8 moment maps (mu_f and G(f^2) shared by the two pairs) in registers, from which
//                           l, cs, the per-pixel loss and, for the gradient, the 4 adjoint maps d/d mu_f, d/d G(f^2), d/d G(f ir),
//                           d/d G(f vis) of that scale follow.  Only the adjoint maps and one partial sum per tile leave the CU.
//   loss_finish_kernel      partial sums -> terms[5] (one block, fp64 accumulation of the few thousand partials).
//   loss_ssim_grad_kernel   applies the adjoint of each scale's filter to its adjoint maps (zero border: the same filter; reflect
//                           border: the border taps folded back inwards) and adds the result to the gradient.
//   loss_psnr_grad_kernel   adds the PSNR gradient, which needs the two mean squared errors first.
#include "kernels_loss.h"

#include <algorithm>
#include <cmath>

namespace swf {
namespace {

constexpr int kTile = 32;
constexpr float kC1 = 1e-4f, kC2 = 9e-4f;   // (0.01 * max_val)^2, (0.03 * max_val)^2 with max_val = 1

// tap d of scale s at g[s][16 + d]; mode 1 uses g[0] with |d| <= 5
struct LossTaps {
    float g[5][33];
};
constexpr int kTapFloats = 5 * 33;
// The taps arrive as a kernel argument and are read from LDS (sT[s * 33 + 16 + d]); the caller's next barrier publishes them.
__device__ __forceinline__ void stage_taps(const LossTaps& taps, float* sT) {
    if (threadIdx.x < kTapFloats) sT[threadIdx.x] = (&taps.g[0][0])[threadIdx.x];
}

template <int MODE>
struct Geom;
template <>
struct Geom<0> {
    static constexpr int NS = 5, HALO = 16, NM = 10;   // maps per scale: f i v ff ii vv fi fv (+ |f-i| |f-v| at the last scale)
};
template <>
struct Geom<1> {
    static constexpr int NS = 1, HALO = 5, NM = 8;
};
// Taps further out than this are below 1e-12 of the centre tap (exp(-d^2 / 2 sigma^2), sigma = 0.5 1 2 4 8) and are skipped.
template <int MODE, int S>
constexpr int radius() {
    return MODE == 1 ? 5 : (S == 0 ? 4 : S == 1 ? 8 : S == 2 ? 15 : 16);
}

__device__ __forceinline__ float sgn(float x) { return x > 0.f ? 1.f : (x < 0.f ? -1.f : 0.f); }
__device__ __forceinline__ int clampi(int i, int n) { return i < 0 ? 0 : (i >= n ? n - 1 : i); }

// Sum of v over the block in a fixed order (tree over LDS); valid in thread 0.  red holds THREADS floats.
template <int THREADS>
__device__ __forceinline__ float block_sum(float v, float* red) {
    const int tid = threadIdx.x;
    red[tid] = v;
    __syncthreads();
#pragma unroll
    for (int s = THREADS / 2; s > 0; s >>= 1) {
        if (tid < s) red[tid] += red[tid + s];
        __syncthreads();
    }
    return red[0];
}

// ------------------------------------------------------------------------------------------------------------------------------
// Texture (Sobel magnitude, replicate border), intensity, squared errors
// ------------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void sobel(const float* p, int stride, float& gx, float& gy) {   // p = top-left of the 3x3 patch
    const float a = p[0], b = p[1], c = p[2], d = p[stride], e = p[stride + 2], f = p[2 * stride], g = p[2 * stride + 1], h = p[2 * stride + 2];
    gx = ((c - a) + 2.f * (e - d) + (h - f)) * 0.125f;
    gy = ((f - a) + 2.f * (g - b) + (h - c)) * 0.125f;
}

// One axis of the adjoint of a 3-tap correlation with replicate border: weight with which d/d out(p) reaches in(q),
// sum over k of coef[k] where clamp(p + k) == q.
__device__ __forceinline__ float fold3(int q, int p, int n, float cm, float c0, float cp) {
    float w = 0.f;
    if (clampi(p - 1, n) == q) w += cm;
    if (p == q) w += c0;
    if (clampi(p + 1, n) == q) w += cp;
    return w;
}

// part[4][blocks]: sum |E_f - max(E_i, E_v)|, sum |f - max(i, v)|, sum (f - i)^2, sum (f - v)^2 of the tile.
// grad (GRAD) <- ct * d/df sum|..E..| + ci * sign(f - max(i, v)), ct = texture coefficient / N, ci = intensity coefficient / N.
template <bool GRAD>
__global__ __launch_bounds__(256) void loss_pointwise_kernel(const float* __restrict__ fus, const float* __restrict__ ir,
                                                             const float* __restrict__ vis, float* __restrict__ part, float* __restrict__ grad,
                                                             int H, int W, float ct, float ci) {
    constexpr int IN = kTile + 4, UD = kTile + 2;
    __shared__ float sIn[3][IN * IN];
    __shared__ float sU[2][UD * UD];
    __shared__ float red[256];
    const int tid = threadIdx.x, x0 = blockIdx.x * kTile, y0 = blockIdx.y * kTile;
    const int64_t img = (int64_t)blockIdx.z * H * W;
    const int nblk = gridDim.x * gridDim.y * gridDim.z, blk = (blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
    for (int idx = tid; idx < IN * IN; idx += 256) {
        const int r = idx / IN, c = idx % IN;
        const int64_t o = img + (int64_t)clampi(y0 + r - 2, H) * W + clampi(x0 + c - 2, W);
        sIn[0][idx] = fus[o];
        sIn[1][idx] = ir[o];
        sIn[2][idx] = vis[o];
    }
    __syncthreads();
    float sT = 0.f, sI = 0.f, sEi = 0.f, sEv = 0.f;
    for (int idx = tid; idx < UD * UD; idx += 256) {
        const int r = idx / UD, c = idx % UD;
        const int py = y0 + r - 1, px = x0 + c - 1;
        float ux = 0.f, uy = 0.f;
        if (py >= 0 && py < H && px >= 0 && px < W) {
            float gx, gy, hx, hy;
            sobel(&sIn[0][r * IN + c], IN, gx, gy);
            const float ef = sqrtf(gx * gx + gy * gy + 1e-6f);
            sobel(&sIn[1][r * IN + c], IN, hx, hy);
            const float ei = sqrtf(hx * hx + hy * hy + 1e-6f);
            sobel(&sIn[2][r * IN + c], IN, hx, hy);
            const float ev = sqrtf(hx * hx + hy * hy + 1e-6f);
            const float dlt = ef - fmaxf(ei, ev);
            const float t = sgn(dlt) / ef;
            ux = t * gx;
            uy = t * gy;
            if (r >= 1 && r <= kTile && c >= 1 && c <= kTile) {
                const int ctr = (r + 1) * IN + c + 1;
                const float f = sIn[0][ctr], a = sIn[1][ctr], b = sIn[2][ctr];
                sT += fabsf(dlt);
                sI += fabsf(f - fmaxf(a, b));
                sEi += (f - a) * (f - a);
                sEv += (f - b) * (f - b);
            }
        }
        sU[0][idx] = ux;
        sU[1][idx] = uy;
    }
    __syncthreads();
    if (GRAD) {
        const int tx = tid % kTile, ty = tid / kTile;
        const int qx = x0 + tx;
        float smx[3], dfx[3];
#pragma unroll
        for (int b = 0; b < 3; ++b) {
            smx[b] = fold3(qx, qx - 1 + b, W, 1.f, 2.f, 1.f);
            dfx[b] = fold3(qx, qx - 1 + b, W, -1.f, 0.f, 1.f);
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int ly = ty + 8 * j, qy = y0 + ly;
            if (qy >= H || qx >= W) continue;
            float g = 0.f;
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                const float smy = fold3(qy, qy - 1 + a, H, 1.f, 2.f, 1.f), dfy = fold3(qy, qy - 1 + a, H, -1.f, 0.f, 1.f);
#pragma unroll
                for (int b = 0; b < 3; ++b) {
                    const int u = (ly + a) * UD + tx + b;   // sU is 0 outside the image
                    g += sU[0][u] * (smy * dfx[b]) + sU[1][u] * (dfy * smx[b]);
                }
            }
            const int ctr = (ly + 2) * IN + tx + 2;
            const float f = sIn[0][ctr], m = fmaxf(sIn[1][ctr], sIn[2][ctr]);
            grad[img + (int64_t)qy * W + qx] = ct * 0.125f * g + ci * sgn(f - m);
        }
    }
    float t;
    t = block_sum<256>(sT, red);
    if (tid == 0) part[blk] = t;
    __syncthreads();
    t = block_sum<256>(sI, red);
    if (tid == 0) part[nblk + blk] = t;
    __syncthreads();
    t = block_sum<256>(sEi, red);
    if (tid == 0) part[2 * nblk + blk] = t;
    __syncthreads();
    t = block_sum<256>(sEv, red);
    if (tid == 0) part[3 * nblk + blk] = t;
}

// ------------------------------------------------------------------------------------------------------------------------------
// SSIM term: moments, per-pixel loss, adjoint maps
// ------------------------------------------------------------------------------------------------------------------------------
// Filtered maps of scale S at this thread's two pixels (rows ty and ty + 16 of the tile, column tx): row pass sIn -> sMid over the
// rows the column taps reach, then the column pass into m[2][NM].
template <int MODE, int S>
__device__ __forceinline__ void scale_moments(const float* sIn, float* sMid, const float* sT, float (&m)[2][Geom<MODE>::NM]) {
    using G = Geom<MODE>;
    constexpr int IN = kTile + 2 * G::HALO, R = radius<MODE, S>();
    constexpr int NMS = (MODE == 0 && S == 4) ? 10 : 8;
    const int tid = threadIdx.x;
    __syncthreads();   // sMid of the previous scale is no longer read
    for (int idx = tid; idx < IN * kTile; idx += 512) {
        const int r = idx / kTile, c = idx % kTile;
        if (r < G::HALO - R || r >= G::HALO + kTile + R) continue;
        float a[NMS];
#pragma unroll
        for (int k = 0; k < NMS; ++k) a[k] = 0.f;
        const float* p = sIn + r * IN + c + G::HALO;
#pragma unroll 1
        for (int d = -R; d <= R; ++d) {
            const float g = sT[S * 33 + 16 + d];
            const float x = p[d], y = p[IN * IN + d], z = p[2 * IN * IN + d];
            a[0] += g * x;
            a[1] += g * y;
            a[2] += g * z;
            a[3] += g * (x * x);
            a[4] += g * (y * y);
            a[5] += g * (z * z);
            a[6] += g * (x * y);
            a[7] += g * (x * z);
            if (NMS == 10) {
                a[8] += g * fabsf(x - y);
                a[9] += g * fabsf(x - z);
            }
        }
#pragma unroll
        for (int k = 0; k < NMS; ++k) sMid[k * IN * kTile + idx] = a[k];
    }
    __syncthreads();
    const int tx = tid % kTile, ty = tid / kTile;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
#pragma unroll
        for (int k = 0; k < NMS; ++k) m[j][k] = 0.f;
        const float* p = sMid + (ty + 16 * j + G::HALO) * kTile + tx;
#pragma unroll 1
        for (int d = -R; d <= R; ++d) {
            const float g = sT[S * 33 + 16 + d];
#pragma unroll
            for (int k = 0; k < NMS; ++k) m[j][k] += g * p[k * IN * kTile + d * kTile];
        }
    }
}

// What the MS-SSIM gradient needs of one scale at one pixel, per pair (0 = ir, 1 = vis)
struct ScaleState {
    float muf, muy[2], cs[2], invb[2];
};

template <int S>
__device__ __forceinline__ void ms_scale(const float* sIn, float* sMid, const float* sT, ScaleState (&st)[5][2], float (&l)[2][2],
                                         float (&invbl)[2][2], float (&l1)[2][2]) {
    float m[2][10];
    scale_moments<0, S>(sIn, sMid, sT, m);
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const float muf = m[j][0], ff = m[j][3] - muf * muf;
        st[S][j].muf = muf;
#pragma unroll
        for (int y = 0; y < 2; ++y) {
            const float muy = m[j][1 + y], yy = m[j][4 + y] - muy * muy, fy = m[j][6 + y] - muf * muy;
            const float invb = 1.f / (ff + yy + kC2);
            st[S][j].muy[y] = muy;
            st[S][j].invb[y] = invb;
            st[S][j].cs[y] = (2.f * fy + kC2) * invb;
            if (S == 4) {
                invbl[j][y] = 1.f / (muf * muf + muy * muy + kC1);
                l[j][y] = (2.f * muf * muy + kC1) * invbl[j][y];
                l1[j][y] = m[j][8 + y];
            }
        }
    }
}

// part[blocks] <- sum over the tile of w_ir * pixel loss(f, ir) + w_vis * pixel loss(f, vis).
// adj (GRAD): [NS][4][N] <- d (coefficient * S) / d {mu_f, G(f^2), G(f ir), G(f vis)} of every scale; gs = coefficient / N.
template <int MODE, bool GRAD>
__global__ __launch_bounds__(512) void loss_moments_kernel(const float* __restrict__ fus, const float* __restrict__ ir,
                                                           const float* __restrict__ vis, float* __restrict__ part, float* __restrict__ adj,
                                                           int H, int W, int64_t N, float wi, float wv, float gs, LossTaps taps) {
    using G = Geom<MODE>;
    constexpr int IN = kTile + 2 * G::HALO;
    extern __shared__ __align__(16) float smem[];
    float* sIn = smem;                    // [3][IN][IN]
    float* sMid = smem + 3 * IN * IN;     // [NM][IN][kTile]
    float* sT = sMid + G::NM * IN * kTile;
    stage_taps(taps, sT);
    const int tid = threadIdx.x, x0 = blockIdx.x * kTile, y0 = blockIdx.y * kTile;
    const int64_t img = (int64_t)blockIdx.z * H * W;
    const int blk = (blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
    for (int idx = tid; idx < IN * IN; idx += 512) {
        const int gy = y0 + idx / IN - G::HALO, gx = x0 + idx % IN - G::HALO;
        float a = 0.f, b = 0.f, c = 0.f;
        if (MODE == 0) {   // zero border
            if (gy >= 0 && gy < H && gx >= 0 && gx < W) {
                const int64_t o = img + (int64_t)gy * W + gx;
                a = fus[o], b = ir[o], c = vis[o];
            }
        } else if (gy < H + G::HALO && gx < W + G::HALO) {   // reflect border (H, W > HALO); further out only masked pixels read
            const int64_t o = img + (int64_t)reflect2(gy, H) * W + reflect2(gx, W);
            a = fus[o], b = ir[o], c = vis[o];
        }
        sIn[idx] = a;
        sIn[IN * IN + idx] = b;
        sIn[2 * IN * IN + idx] = c;
    }
    // (scale_moments begins with a barrier)
    const int tx = tid % kTile, ty = tid / kTile;
    const float w[2] = {wi, wv};
    float val = 0.f;
    if constexpr (MODE == 0) {
        ScaleState st[5][2];
        float l[2][2], invbl[2][2], l1[2][2];
        ms_scale<0>(sIn, sMid, sT, st, l, invbl, l1);
        ms_scale<1>(sIn, sMid, sT, st, l, invbl, l1);
        ms_scale<2>(sIn, sMid, sT, st, l, invbl, l1);
        ms_scale<3>(sIn, sMid, sT, st, l, invbl, l1);
        ms_scale<4>(sIn, sMid, sT, st, l, invbl, l1);
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int qy = y0 + ty + 16 * j, qx = x0 + tx;
            if (qy >= H || qx >= W) continue;
            const int64_t o = img + (int64_t)qy * W + qx;
            float amu[5], aff[5], afy[5][2];
#pragma unroll
            for (int s = 0; s < 5; ++s) amu[s] = aff[s] = 0.f;
#pragma unroll
            for (int y = 0; y < 2; ++y) {
                float c3[5], pics = 1.f;
#pragma unroll
                for (int s = 0; s < 5; ++s) {
                    const float c = st[s][j].cs[y];
                    c3[s] = c * c * c;
                    pics *= c3[s];
                }
                const float lm = l[j][y] * l[j][y] * l[j][y];
                val += w[y] * (200.f * (0.025f * (1.f - lm * pics) + 0.975f * l1[j][y]));
                if (GRAD) {
                    const float k = -5.f * gs * w[y];   // d / d (l^3 * prod cs^3): 200 * 0.025 = 5
#pragma unroll
                    for (int s = 0; s < 5; ++s) {
                        float others = 1.f;
#pragma unroll
                        for (int t = 0; t < 5; ++t)
                            if (t != s) others *= c3[t];
                        const float c = st[s][j].cs[y], invb = st[s][j].invb[y];
                        const float dcs = k * lm * 3.f * c * c * others;
                        aff[s] += dcs * (-c * invb);
                        afy[s][y] = dcs * 2.f * invb;
                        amu[s] += dcs * (2.f * c * st[s][j].muf - 2.f * st[s][j].muy[y]) * invb;
                    }
                    const float dl = k * 3.f * l[j][y] * l[j][y] * pics;
                    amu[4] += dl * (2.f * st[4][j].muy[y] - 2.f * l[j][y] * st[4][j].muf) * invbl[j][y];
                }
            }
            if (GRAD) {
#pragma unroll
                for (int s = 0; s < 5; ++s) {
                    adj[(s * 4 + 0) * N + o] = amu[s];
                    adj[(s * 4 + 1) * N + o] = aff[s];
                    adj[(s * 4 + 2) * N + o] = afy[s][0];
                    adj[(s * 4 + 3) * N + o] = afy[s][1];
                }
            }
        }
    } else {
        float m[2][8];
        scale_moments<1, 0>(sIn, sMid, sT, m);
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int qy = y0 + ty + 16 * j, qx = x0 + tx;
            if (qy >= H || qx >= W) continue;
            const int64_t o = img + (int64_t)qy * W + qx;
            const float muf = m[j][0], ff = m[j][3] - muf * muf;
            float amu = 0.f, aff = 0.f, afy[2];
#pragma unroll
            for (int y = 0; y < 2; ++y) {
                const float muy = m[j][1 + y], yy = m[j][4 + y] - muy * muy, fy = m[j][6 + y] - muf * muy;
                const float a1 = 2.f * muf * muy + kC1, b1 = muf * muf + muy * muy + kC1, a2 = 2.f * fy + kC2, b2 = ff + yy + kC2;
                const float iden = 1.f / (b1 * b2 + 1e-12f);
                const float ssim = a1 * a2 * iden;
                const float dd = 0.5f * (1.f - ssim);
                val += w[y] * 2.f * fminf(fmaxf(dd, 0.f), 1.f);
                if (GRAD) {
                    const float g0 = (dd >= 0.f && dd <= 1.f) ? -gs * w[y] : 0.f;   // d / d ssim
                    const float da1 = g0 * a2 * iden, da2 = g0 * a1 * iden, db1 = -g0 * ssim * b2 * iden, db2 = -g0 * ssim * b1 * iden;
                    amu += 2.f * muy * (da1 - da2) + 2.f * muf * (db1 - db2);
                    aff += db2;
                    afy[y] = 2.f * da2;
                }
            }
            if (GRAD) {
                adj[o] = amu;
                adj[N + o] = aff;
                adj[2 * N + o] = afy[0];
                adj[3 * N + o] = afy[1];
            }
        }
    }
    __syncthreads();   // sMid becomes the reduction buffer
    const float t = block_sum<512>(val, sMid);
    if (tid == 0) part[blk] = t;
}

// ------------------------------------------------------------------------------------------------------------------------------
// SSIM term: adjoint filters
// ------------------------------------------------------------------------------------------------------------------------------
// One axis of the adjoint of the scale's filter: weight with which the adjoint at p = q + d reaches the input at q (axis length n).
// Zero border: the tap itself.  Reflect border: plus the taps of the padded positions -q and 2n - 2 - q that mirror onto q.
template <int MODE, int R>
__device__ __forceinline__ float adjoint_tap(const float* g, int q, int d, int n) {
    float w = g[16 + d];
    if (MODE == 1) {
        const int e1 = 2 * q + d, e2 = 2 * n - 2 - 2 * q - d;   // (-q) - p and (2n - 2 - q) - p
        if (q >= 1 && q <= R && e1 >= -R && e1 <= R) w += g[16 + e1];
        if (q >= n - 1 - R && q <= n - 2 && e2 >= -R && e2 <= R) w += g[16 + e2];
    }
    return w;
}

template <int MODE, int S>
__device__ __forceinline__ void scale_adjoint(const float* __restrict__ adj, float* sA, float* sMid, const float* sT, int H, int W,
                                              int64_t N, int64_t img, int x0, int y0, const float (&mul)[4][3], float (&acc)[4]) {
    using G = Geom<MODE>;
    constexpr int IN = kTile + 2 * G::HALO, R = radius<MODE, S>(), LO = G::HALO - R, HI = G::HALO + kTile + R;
    const int tid = threadIdx.x, tx = tid % kTile, ty = tid / kTile;
    for (int m = 0; m < 4; ++m) {
        const float* map = adj + (S * 4 + m) * N + img;
        for (int idx = tid; idx < IN * IN; idx += 256) {
            const int r = idx / IN, c = idx % IN;
            if (r < LO || r >= HI || c < LO || c >= HI) continue;
            const int gy = y0 + r - G::HALO, gx = x0 + c - G::HALO;
            sA[idx] = (gy >= 0 && gy < H && gx >= 0 && gx < W) ? map[(int64_t)gy * W + gx] : 0.f;
        }
        __syncthreads();   // also: every column pass over sMid of the previous map is done
        for (int idx = tid; idx < IN * kTile; idx += 256) {
            const int r = idx / kTile, c = idx % kTile;
            if (r < LO || r >= HI) continue;
            const float* p = sA + r * IN + c + G::HALO;
            float a = 0.f;
#pragma unroll 1
            for (int d = -R; d <= R; ++d) a += p[d] * adjoint_tap<MODE, R>(sT + S * 33, x0 + c, d, W);
            sMid[idx] = a;
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int ly = ty + 8 * j;
            const float* p = sMid + (ly + G::HALO) * kTile + tx;
            float a = 0.f;
#pragma unroll 1
            for (int d = -R; d <= R; ++d) a += p[d * kTile] * adjoint_tap<MODE, R>(sT + S * 33, y0 + ly, d, H);
            acc[j] += (m == 0 ? 1.f : mul[j][m - 1]) * a;
        }
    }
}

// grad += sum over scales of G'(a_mu) + 2 f G'(a_ff) + ir G'(a_fi) + vis G'(a_fv), G' the adjoint filter; mode 0 adds the L1 part,
// (l1i sign(f - ir) + l1v sign(f - vis)) * G_8'(1), whose filtered map of ones is the product of two 1-D border sums.
template <int MODE>
__global__ __launch_bounds__(256) void loss_ssim_grad_kernel(const float* __restrict__ fus, const float* __restrict__ ir,
                                                             const float* __restrict__ vis, const float* __restrict__ adj,
                                                             float* __restrict__ grad, int H, int W, int64_t N, float l1i, float l1v, LossTaps taps) {
    using G = Geom<MODE>;
    constexpr int IN = kTile + 2 * G::HALO;
    __shared__ float sA[IN * IN];
    __shared__ float sMid[IN * kTile];
    __shared__ float sCw[2][kTile];
    __shared__ float sT[kTapFloats];
    const int tid = threadIdx.x, tx = tid % kTile, ty = tid / kTile, x0 = blockIdx.x * kTile, y0 = blockIdx.y * kTile;
    const int64_t img = (int64_t)blockIdx.z * H * W;
    stage_taps(taps, sT);
    __syncthreads();
    if (MODE == 0 && tid < 2 * kTile) {
        const int axis = tid / kTile, q = (axis ? y0 : x0) + tid % kTile, n = axis ? H : W;
        float s = 0.f;
        for (int d = -16; d <= 16; ++d)
            if (q + d >= 0 && q + d < n) s += sT[4 * 33 + 16 + d];
        sCw[axis][tid % kTile] = s;
    }
    float mul[4][3], acc[4] = {0.f, 0.f, 0.f, 0.f};
    const int qx = x0 + tx;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int qy = y0 + ty + 8 * j;
        const bool in = qy < H && qx < W;
        const int64_t o = img + (int64_t)qy * W + qx;
        mul[j][0] = in ? 2.f * fus[o] : 0.f;
        mul[j][1] = in ? ir[o] : 0.f;
        mul[j][2] = in ? vis[o] : 0.f;
    }
    scale_adjoint<MODE, 0>(adj, sA, sMid, sT, H, W, N, img, x0, y0, mul, acc);
    if constexpr (MODE == 0) {
        scale_adjoint<0, 1>(adj, sA, sMid, sT, H, W, N, img, x0, y0, mul, acc);
        scale_adjoint<0, 2>(adj, sA, sMid, sT, H, W, N, img, x0, y0, mul, acc);
        scale_adjoint<0, 3>(adj, sA, sMid, sT, H, W, N, img, x0, y0, mul, acc);
        scale_adjoint<0, 4>(adj, sA, sMid, sT, H, W, N, img, x0, y0, mul, acc);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int ly = ty + 8 * j, qy = y0 + ly;
        if (qy >= H || qx >= W) continue;
        const int64_t o = img + (int64_t)qy * W + qx;
        float g = acc[j];
        if (MODE == 0) {
            const float f = 0.5f * mul[j][0];
            g += (l1i * sgn(f - mul[j][1]) + l1v * sgn(f - mul[j][2])) * (sCw[0][tx] * sCw[1][ly]);
        }
        grad[o] += g;
    }
}

// scal[0..1] = mse(f, ir), mse(f, vis); kp = psnr coefficient * 20 / (ln 10 * N)
__global__ __launch_bounds__(256) void loss_psnr_grad_kernel(const float* __restrict__ fus, const float* __restrict__ ir,
                                                             const float* __restrict__ vis, const float* __restrict__ scal,
                                                             float* __restrict__ grad, int64_t N, float kp, float wi, float wv) {
    const float ci = kp * wi / scal[0], cv = kp * wv / scal[1];
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < N; i += (int64_t)gridDim.x * 256) {
        const float f = fus[i];
        grad[i] += ci * (f - ir[i]) + cv * (f - vis[i]);
    }
}

struct LossCoef {
    float cs, ct, ci, cp, wpi, wpv;
    int use_psnr;
};

// terms <- S, T, I, P, total from the per-tile partial sums: every thread adds its strided share in order, then a tree.
__global__ __launch_bounds__(256) void loss_finish_kernel(const float* __restrict__ part_s, const float* __restrict__ part_p, int nblk,
                                                          double inv_n, LossCoef k, float* __restrict__ terms, float* __restrict__ scal) {
    __shared__ double red[5][256];
    const int tid = threadIdx.x;
    double a[5] = {0, 0, 0, 0, 0};
    for (int i = tid; i < nblk; i += 256) {
        a[0] += part_s[i];
#pragma unroll
        for (int t = 0; t < 4; ++t) a[1 + t] += part_p[t * nblk + i];
    }
#pragma unroll
    for (int t = 0; t < 5; ++t) red[t][tid] = a[t];
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (tid < s)
#pragma unroll
            for (int t = 0; t < 5; ++t) red[t][tid] += red[t][tid + s];
        __syncthreads();
    }
    if (tid == 0) {
        const double S = red[0][0] * inv_n, T = red[1][0] * inv_n, I = red[2][0] * inv_n, mi = red[3][0] * inv_n, mv = red[4][0] * inv_n;
        const double P = k.use_psnr ? 10.0 * (k.wpi * log10(mi) + k.wpv * log10(mv)) : 0.0;   // -10 log10(1 / mse)
        terms[0] = (float)S;
        terms[1] = (float)T;
        terms[2] = (float)I;
        terms[3] = (float)P;
        terms[4] = (float)(k.cs * S + k.ct * T + k.ci * I + k.cp * P);
        scal[0] = (float)mi;
        scal[1] = (float)mv;
    }
}

struct TapTables {
    LossTaps t[2];
    TapTables() {
        std::memset(t, 0, sizeof t);
        const double sigmas[5] = {0.5, 1.0, 2.0, 4.0, 8.0};
        for (int s = 0; s < 5; ++s) fill(t[0].g[s], 16, sigmas[s]);
        fill(t[1].g[0], 5, 1.5);
    }
    // g[16 + d] = exp(-d^2 / 2 sigma^2) / sum, |d| <= r, in fp64 and rounded once
    static void fill(float* g, int r, double sigma) {
        double e[33], sum = 0;
        for (int d = -r; d <= r; ++d) sum += e[d + r] = std::exp(-double(d * d) / (2.0 * sigma * sigma));
        for (int d = -r; d <= r; ++d) g[16 + d] = float(e[d + r] / sum);
    }
};
const LossTaps& loss_taps(int mode) {
    static const TapTables tables;
    return tables.t[mode];
}

dim3 tile_grid(int B, int H, int W) { return dim3(cdiv(W, kTile), cdiv(H, kTile), B); }

template <int MODE>
constexpr int moments_lds_bytes() {
    constexpr int IN = kTile + 2 * Geom<MODE>::HALO;
    return (3 * IN * IN + Geom<MODE>::NM * IN * kTile + kTapFloats) * (int)sizeof(float);
}

template <int MODE, bool GRAD>
int launch_moments(const float* f, const float* ir, const float* vis, float* part, float* adj, int B, int H, int W, float wi, float wv,
                   float gs, hipStream_t stream) {
    constexpr int lds = moments_lds_bytes<MODE>();
    SWF_TRY((raise_lds_limit<loss_moments_kernel<MODE, GRAD>>(lds, "loss_moments_kernel")));
    loss_moments_kernel<MODE, GRAD><<<tile_grid(B, H, W), 512, lds, stream>>>(f, ir, vis, part, adj, H, W, (int64_t)B * H * W, wi, wv, gs,
                                                                             loss_taps(MODE));
    return check_launch("loss_moments_kernel");
}

struct LossBuffers {
    float *part_s, *part_p, *scal, *adj;
};
LossBuffers carve_loss(Carver& cv, const swf_loss_desc& d, int B, int H, int W, bool with_grad) {
    const int64_t nblk = (int64_t)cdiv(W, kTile) * cdiv(H, kTile) * B, n = (int64_t)B * H * W;
    LossBuffers b;
    b.part_s = cv.floats(nblk);
    b.part_p = cv.floats(4 * nblk);
    b.scal = cv.floats(4);
    const bool ssim_grad = with_grad && d.ssim_ratio * d.ssim_scale != 0.f;
    b.adj = ssim_grad ? cv.floats((d.ssim_mode == 0 ? 5 : 1) * 4 * n) : nullptr;
    return b;
}

}  // namespace

size_t fusion_loss_workspace_bytes(const swf_loss_desc& d, int B, int H, int W, bool with_grad) {
    Carver cv = Carver::measure();
    carve_loss(cv, d, B, H, W, with_grad);
    return cv.bytes();
}

int fusion_loss(const swf_loss_desc& d, const float* fusion, const float* ir, const float* vis, float* terms, float* grad,
                int B, int H, int W, void* workspace, size_t workspace_bytes, hipStream_t stream) {
    Carver cv(workspace, workspace_bytes);
    const LossBuffers b = carve_loss(cv, d, B, H, W, grad != nullptr);
    if (!cv.ok()) return fail(SWF_ERR_WORKSPACE, "fusion_loss: workspace too small (%zu < %zu bytes)", workspace_bytes, cv.bytes());
    const int64_t n = (int64_t)B * H * W;
    const double inv_n = 1.0 / double(n);
    LossCoef k;
    k.cs = d.ssim_ratio * d.ssim_scale;
    k.ct = d.texture_ratio * d.texture_scale;
    k.ci = d.intensity_ratio * d.intensity_scale;
    k.cp = d.use_psnr ? d.psnr_ratio * d.psnr_scale : 0.f;
    k.wpi = d.ir_psnr_weight;
    k.wpv = 1.f - d.ir_psnr_weight;
    k.use_psnr = d.use_psnr != 0;
    const float wi = d.ir_ssim_weight, wv = 1.f - d.ir_ssim_weight;
    const dim3 grid = tile_grid(B, H, W);
    const int nblk = (int)(grid.x * grid.y * grid.z);

    if (grad)
        loss_pointwise_kernel<true><<<grid, 256, 0, stream>>>(fusion, ir, vis, b.part_p, grad, H, W, float(k.ct * inv_n), float(k.ci * inv_n));
    else
        loss_pointwise_kernel<false><<<grid, 256, 0, stream>>>(fusion, ir, vis, b.part_p, nullptr, H, W, 0.f, 0.f);
    SWF_TRY(check_launch("loss_pointwise_kernel"));

    const float gs = float(k.cs * inv_n);
    if (d.ssim_mode == 0)
        SWF_TRY(b.adj ? (launch_moments<0, true>(fusion, ir, vis, b.part_s, b.adj, B, H, W, wi, wv, gs, stream))
                      : (launch_moments<0, false>(fusion, ir, vis, b.part_s, nullptr, B, H, W, wi, wv, gs, stream)));
    else
        SWF_TRY(b.adj ? (launch_moments<1, true>(fusion, ir, vis, b.part_s, b.adj, B, H, W, wi, wv, gs, stream))
                      : (launch_moments<1, false>(fusion, ir, vis, b.part_s, nullptr, B, H, W, wi, wv, gs, stream)));

    loss_finish_kernel<<<1, 256, 0, stream>>>(b.part_s, b.part_p, nblk, inv_n, k, terms, b.scal);
    SWF_TRY(check_launch("loss_finish_kernel"));

    if (b.adj) {
        if (d.ssim_mode == 0)   // 200 * 0.975 = 195: the Gaussian-weighted L1 of MS_SSIMLoss
            loss_ssim_grad_kernel<0><<<grid, 256, 0, stream>>>(fusion, ir, vis, b.adj, grad, H, W, n, 195.f * gs * wi, 195.f * gs * wv, loss_taps(0));
        else
            loss_ssim_grad_kernel<1><<<grid, 256, 0, stream>>>(fusion, ir, vis, b.adj, grad, H, W, n, 0.f, 0.f, loss_taps(1));
        SWF_TRY(check_launch("loss_ssim_grad_kernel"));
    }
    if (grad && k.cp != 0.f) {
        const int blocks = (int)std::min<int64_t>(cdiv64(n, 256), 4096);
        loss_psnr_grad_kernel<<<blocks, 256, 0, stream>>>(fusion, ir, vis, b.scal, grad, n, float(k.cp * 20.0 / std::log(10.0) * inv_n), k.wpi, k.wpv);
        SWF_TRY(check_launch("loss_psnr_grad_kernel"));
    }
    return SWF_OK;
}

}  // namespace swf
