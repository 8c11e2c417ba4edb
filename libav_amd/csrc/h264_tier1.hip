/*
 * h264_tier1.hip — Tier-1 entry points: the reference's H.264 DSP pointer tables
 * (H264DSPContext, H264QpelContext, H264ChromaContext, H264PredContext,
 * VideoDSPContext) served by HIP kernels, one synchronous launch per call, for the
 * BIT_DEPTH 8, 9 and 10 instantiations of the reference's templates (h264dsp.c:37-47,
 * :57-135; h264qpel.c:47-100; h264chroma.c:35-52; h264pred.c:408-565; videodsp.c:35-42).
 * Above 8 bit samples are 16-bit (`pixel` = uint16_t) and coefficients 32-bit (`dctcoef`
 * = int32_t behind the tables' int16_t pointers); strides stay in bytes.
 *
 * Host side = gather the touched sample window + parameters into the staging
 * arena, launch, scatter the written extent back, and reproduce the reference's
 * side effects on the coefficient block (cleared after use, h264idct_template.c:66,
 * :140, :150, :164).  Every shim is written once for the three depths: widths and
 * x-offsets are in samples, times sizeof(PX) where bytes are needed; pitches handed
 * to kernels are in samples.
 *
 * All arithmetic runs in the kernels.  The loop-filter lines, the intra predictors,
 * the lossless adds and the edge emulation are one template per sample type.  Motion
 * compensation, the inverse transforms, the DC transforms and weighted prediction have
 * TWO forms behind one shim: at 8 bit thin wrappers over the same wave-level building
 * blocks (h264_dev.h) the batched frame pipeline uses, so parity here is parity of the
 * hot path's arithmetic; at 9 / 10 bit (k_hbd_*) the integer formulation of the
 * reference's templates with the bit depth as a parameter.  These tables are the
 * per-call (slow) boundary: what matters at 9 / 10 bit is that a High 10 stream decodes
 * through the device bit-exactly, not the rate.
 */
#include "mi355_rt.h"
#include "h264_dev.h"
#include "../../include/mi355dsp.h"
#include <type_traits>

using namespace mi355;

#define LAUNCH1(kernel, a, ...) \
    hipLaunchKernelGGL(kernel, dim3(1), dim3(64), 0, (a).stream, __VA_ARGS__)

/* sample (`pixel`) and coefficient (`dctcoef`) types of a bit depth, and the sample range */
template <typename PX> using CoefOf = typename std::conditional<sizeof(PX) == 1, int16_t, int32_t>::type;
template <int BD> struct Smp {
    typedef typename std::conditional<BD == 8, uint8_t, uint16_t>::type PX;
    typedef CoefOf<PX> COEF;
    static constexpr int MAXV = (1 << BD) - 1;
};
template <int BD> using Px = typename Smp<BD>::PX;
template <int BD> using Coef = typename Smp<BD>::COEF;

/* ------------------------------------------------------------------------- */
/* qpel / chroma MC: h264qpel_template.c:77-300 (6-tap, 16 quarter positions), */
/* h264chroma_template.c:28-200                                                */
/* ------------------------------------------------------------------------- */
__global__ void __launch_bounds__(64)
k_qpel(const uint8_t *win, int wpitch, uint8_t *dst, int dpitch, int size, int mx, int my, int avg)
{
    __shared__ McScratch s;
    __shared__ uint8_t pred[16 * 16];
    const int lane = lane_id();
    if (avg)
        for (int i = lane; i < size * size; i += 64) {
            int y = i / size, x = i - y * size;
            pred[y * 16 + x] = dst[y * dpitch + x];
        }
    __syncthreads();
    PlaneRef ref{win, wpitch, size + 5, size + 5};
    stage_windows(s, &ref, 2, 2, size, size, nullptr, nullptr, 0, 0, 0, 0);
    mc_luma_compute(s, mx, my, size, size, pred, 16, 0, 0, avg);
    for (int i = lane; i < size * size; i += 64) {
        int y = i / size, x = i - y * size;
        dst[y * dpitch + x] = pred[y * 16 + x];
    }
}
__global__ void __launch_bounds__(64)
k_hbd_qpel(const uint16_t *win, int wp, uint16_t *dst, int dp, int size, int mx, int my, int avg, int maxv)
{
    /* window sample (x, y) of the block sits at win[(y + 2) * wp + x + 2] */
#define S(x, y) ((int)win[((y) + 2) * wp + (x) + 2])
    for (int i = lane_id(); i < size * size; i += 64) {
        const int y = i / size, x = i - y * size;
        auto rawh = [&](int xx, int yy) { return tap6(S(xx - 2, yy), S(xx - 1, yy), S(xx, yy), S(xx + 1, yy), S(xx + 2, yy), S(xx + 3, yy)); };
        auto hh = [&](int xx, int yy) { return clip3((rawh(xx, yy) + 16) >> 5, 0, maxv); };
        auto vv = [&](int xx, int yy) { return clip3((tap6(S(xx, yy - 2), S(xx, yy - 1), S(xx, yy), S(xx, yy + 1), S(xx, yy + 2), S(xx, yy + 3)) + 16) >> 5, 0, maxv); };
        /* the reference keeps the first pass of the 2-D positions in int16_t, biased by `pad` at 10 bit (h264qpel_template.c:119-146):
         * samples inside the bit depth's range fit, samples outside it (planes of transform-bypass streams, whose residual adds do
         * not clip) wrap — and so does this */
        const int pad = maxv > 511 ? -10 * maxv : 0;
        auto tmph = [&](int xx, int yy) { return (int)(int16_t)(rawh(xx, yy) + pad) - pad; };
        auto hv = [&](int xx, int yy) {
            return clip3((tap6(tmph(xx, yy - 2), tmph(xx, yy - 1), tmph(xx, yy), tmph(xx, yy + 1), tmph(xx, yy + 2), tmph(xx, yy + 3)) + 512) >> 10, 0, maxv);
        };
        int v;
        if (my == 0) v = mx == 0 ? S(x, y) : (mx == 2 ? hh(x, y) : f2(S(x + (mx == 3), y), hh(x, y)));
        else if (mx == 0) v = my == 2 ? vv(x, y) : f2(S(x, y + (my == 3)), vv(x, y));
        else if (mx == 2 && my == 2) v = hv(x, y);
        else if (mx == 2) v = f2(hh(x, y + (my == 3)), hv(x, y));
        else if (my == 2) v = f2(vv(x + (mx == 3), y), hv(x, y));
        else v = f2(hh(x, y + (my == 3)), vv(x + (mx == 3), y));
        dst[y * dp + x] = (uint16_t)(avg ? f2(dst[y * dp + x], v) : v);
    }
#undef S
}

template <int SIZE, int POS, int AVG, int BD>
static void qpel_shim(uint8_t *dst, const uint8_t *src, ptrdiff_t stride)
{
    using PX = Px<BD>;
    constexpr int B = sizeof(PX);
    Arena &a = arena();
    constexpr int mx = POS & 3, my = POS >> 2;
    /* rows/cols the reference position actually reads (h264qpel_template.c:380-531):
     * copy the full (SIZE+5)^2 apron only where it exists for this position */
    const int x0 = mx ? -2 : 0, x1 = mx ? SIZE + 3 : SIZE;
    const int y0 = my ? -2 : 0, y1 = my ? SIZE + 3 : SIZE;
    Win w = win_pack(a, nullptr, 0, (SIZE + 5) * B, SIZE + 5, 0, 0); /* zero-filled */
    uint8_t *wp = a.h<uint8_t>(w.off);
    if ((mx & 1) && (my & 1)) {
        /* the diagonal quarter positions average one horizontally and one vertically filtered half sample
         * (h264qpel_template.c:429-481: mc11 / mc31 / mc13 / mc33): the reference reads a cross — SIZE rows with the
         * horizontal apron and SIZE columns with the vertical one — and never the four 2 x 2 / 2 x 3 corners */
        const int hrow = my == 3, vcol = mx == 3;          /* mc13 / mc33 filter the rows below, mc31 / mc33 the columns to the right */
        for (int y = hrow; y < hrow + SIZE; y++)
            std::memcpy(wp + (size_t)(y + 2) * w.pitch, src + y * stride - 2 * B, (size_t)(SIZE + 5) * B);
        for (int y = -2; y < SIZE + 3; y++)
            std::memcpy(wp + (size_t)(y + 2) * w.pitch + (2 + vcol) * B, src + y * stride + vcol * B, (size_t)SIZE * B);
    } else
    for (int y = y0; y < y1; y++)
        std::memcpy(wp + (size_t)(y + 2) * w.pitch + (x0 + 2) * B, src + y * stride + x0 * B, (size_t)(x1 - x0) * B);
    Win d = win_pack(a, dst, stride, SIZE * B, SIZE);
    a.upload();
    if constexpr (BD == 8) LAUNCH1(k_qpel, a, a.d<PX>(w.off), w.pitch, a.d<PX>(d.off), d.pitch, SIZE, mx, my, AVG);
    else LAUNCH1(k_hbd_qpel, a, a.d<PX>(w.off), w.pitch / B, a.d<PX>(d.off), d.pitch / B, SIZE, mx, my, AVG, Smp<BD>::MAXV);
    a.download();
    win_unpack(a, d, dst, stride, 0, 0, SIZE * B, SIZE);
}

__global__ void __launch_bounds__(64)
k_chroma(const uint8_t *win, int wpitch, uint8_t *dst, int dpitch, int w, int h, int fx, int fy, int avg)
{
    __shared__ McScratch s;
    __shared__ uint8_t pred[16 * 8];
    const int lane = lane_id();
    if (avg)
        for (int i = lane; i < w * h; i += 64) {
            int y = i / w, x = i - y * w;
            pred[y * 8 + x] = dst[y * dpitch + x];
        }
    __syncthreads();
    PlaneRef ref{win, wpitch, w + 1, h + 1};
    /* h can be 16 (4:2:2 callers); the wave handles it in two 8-row halves */
    for (int y0 = 0; y0 < h; y0 += 8) {
        int bh = h - y0 < 8 ? h - y0 : 8;
        stage_windows(s, nullptr, 0, 0, 0, 0, &ref, &ref, 0, y0, w, bh);
        mc_chroma_compute(s, 1, fx, fy, w, bh, pred, pred, 8, 0, y0, avg);
    }
    for (int i = lane; i < w * h; i += 64) {
        int y = i / w, x = i - y * w;
        dst[y * dpitch + x] = pred[y * 8 + x];
    }
}
__global__ void __launch_bounds__(64)
k_hbd_chroma(const uint16_t *win, int wp, uint16_t *dst, int dp, int w, int h, int fx, int fy, int avg)
{
    const int A = (8 - fx) * (8 - fy), B = fx * (8 - fy), C = (8 - fx) * fy, D = fx * fy;
    for (int i = lane_id(); i < w * h; i += 64) {
        const int y = i / w, x = i - y * w;
        const int v = (A * win[y * wp + x] + B * win[y * wp + x + 1] + C * win[(y + 1) * wp + x] + D * win[(y + 1) * wp + x + 1] + 32) >> 6;
        dst[y * dp + x] = (uint16_t)(avg ? f2(dst[y * dp + x], v) : v);
    }
}

template <int W, int AVG, int BD>
static void chroma_shim(uint8_t *dst, uint8_t *src, ptrdiff_t stride, int h, int x, int y)
{
    using PX = Px<BD>;
    constexpr int B = sizeof(PX);
    Arena &a = arena();
    /* the reference never touches the extra column/row when its weight is zero */
    Win w = win_pack(a, src, stride, (W + 1) * B, h + 1, (x ? W + 1 : W) * B, y ? h + 1 : h);
    Win d = win_pack(a, dst, stride, W * B, h);
    a.upload();
    if constexpr (BD == 8) LAUNCH1(k_chroma, a, a.d<PX>(w.off), w.pitch, a.d<PX>(d.off), d.pitch, W, h, x, y, AVG);
    else LAUNCH1(k_hbd_chroma, a, a.d<PX>(w.off), w.pitch / B, a.d<PX>(d.off), d.pitch / B, W, h, x, y, AVG);
    a.download();
    win_unpack(a, d, dst, stride, 0, 0, W * B, h);
}

/* ------------------------------------------------------------------------- */
/* inverse transforms: h264idct_template.c:33-172                              */
/* ------------------------------------------------------------------------- */
/* up to 16 4x4 or 4 8x8 blocks of one plane window per launch: mode[b] 0 = skip, 1 = dc only, 2 = full; block b
 * is added at sample (bx[b], by[b]) of the window; coefficients coef[b * size * size ..] */
template <typename COEF> struct IdctJob {
    COEF coef[16 * 16];
    uint8_t mode[16], bx[16], by[16];
    int32_t n, size;
};
__global__ void __launch_bounds__(64)
k_idct4(uint8_t *win, int pitch, const IdctJob<int16_t> *job)
{
    const int lane = lane_id(), b = lane >> 2, q = lane & 3;
    int c[4], r[4], row;
    for (int i = 0; i < 4; i++) c[i] = job->coef[b * 16 + q + 4 * i];
    const int mode = job->mode[b];
    idct4_quad(c, q, r, row);
    if (mode == 1) { /* h264idct_template.c:144-156 */
        int dc = (job->coef[b * 16] + 32) >> 6;
        r[0] = r[1] = r[2] = r[3] = dc;
    }
    if (mode)
        add_row4(win + (job->by[b] + row) * pitch + job->bx[b], r);
}
__global__ void __launch_bounds__(64)
k_idct8(uint8_t *win, int pitch, const IdctJob<int16_t> *job)
{
    __shared__ int16_t blk[4 * 64];
    const int lane = lane_id(), b = (lane >> 3) & 3, i = lane & 7;
    for (int k = lane; k < 256; k += 64) blk[k] = job->coef[k];
    __syncthreads();
    const bool active = lane < 32;
    const int mode = job->mode[b];
    int r[8];
    idct8_lds(blk + b * 64, i, active, r);
    if (active && mode) {
        if (mode == 1) { /* h264idct_template.c:159-171 */
            int dc = (job->coef[b * 64] + 32) >> 6;
            for (int k = 0; k < 8; k++) r[k] = dc;
        }
        add_col(win + job->by[b] * pitch + job->bx[b] + i, pitch, r, 8);
    }
}
__device__ inline void hbd_idct4(const int32_t *c, int r[16])
{
    int t[16];
    for (int i = 0; i < 4; i++) {
        const int c0 = c[i] + (i == 0 ? 32 : 0);
        const int z0 = c0 + c[i + 8], z1 = c0 - c[i + 8], z2 = (c[i + 4] >> 1) - c[i + 12], z3 = c[i + 4] + (c[i + 12] >> 1);
        t[i] = z0 + z3; t[i + 4] = z1 + z2; t[i + 8] = z1 - z2; t[i + 12] = z0 - z3;
    }
    for (int i = 0; i < 4; i++) {
        const int z0 = t[4 * i] + t[4 * i + 2], z1 = t[4 * i] - t[4 * i + 2], z2 = (t[4 * i + 1] >> 1) - t[4 * i + 3], z3 = t[4 * i + 1] + (t[4 * i + 3] >> 1);
        /* residual of column i, rows 0..3 */
        r[i] = (z0 + z3) >> 6; r[4 + i] = (z1 + z2) >> 6; r[8 + i] = (z1 - z2) >> 6; r[12 + i] = (z0 - z3) >> 6;
    }
}
__global__ void __launch_bounds__(64) k_hbd_idct(uint16_t *win, int pitch, const IdctJob<int32_t> *job, int maxv)
{
    const int b = lane_id();
    if (b >= job->n || !job->mode[b]) return;
    uint16_t *d = win + job->by[b] * pitch + job->bx[b];
    if (job->size == 4) {
        int r[16];
        if (job->mode[b] == 1) { const int dc = (job->coef[b * 16] + 32) >> 6; for (int k = 0; k < 16; k++) r[k] = dc; }
        else hbd_idct4(job->coef + b * 16, r);
        for (int y = 0; y < 4; y++)
            for (int x = 0; x < 4; x++) d[y * pitch + x] = (uint16_t)clip3(d[y * pitch + x] + r[4 * y + x], 0, maxv);
        return;
    }
    const int32_t *c = job->coef + b * 64;
    if (job->mode[b] == 1) {
        const int dc = (c[0] + 32) >> 6;
        for (int y = 0; y < 8; y++)
            for (int x = 0; x < 8; x++) d[y * pitch + x] = (uint16_t)clip3(d[y * pitch + x] + dc, 0, maxv);
        return;
    }
    int t[64];
    for (int i = 0; i < 8; i++) {          /* first pass over block[i + 8 * k], second over block[k + 8 * i] (:84-134) */
        int in[8], out[8];
        for (int k = 0; k < 8; k++) in[k] = c[i + 8 * k] + ((i == 0 && k == 0) ? 32 : 0);
        idct8_1d(in, out);
        for (int k = 0; k < 8; k++) t[i + 8 * k] = out[k];
    }
    for (int i = 0; i < 8; i++) {
        int in[8], out[8];
        for (int k = 0; k < 8; k++) in[k] = t[k + 8 * i];
        idct8_1d(in, out);
        for (int k = 0; k < 8; k++) d[k * pitch + i] = (uint16_t)clip3(d[k * pitch + i] + (out[k] >> 6), 0, maxv);
    }
}

/* run up to 16 4x4 or 4 8x8 jobs against one destination plane window */
template <typename COEF> struct BlockReq {
    int off;        /* byte offset of the block from `dst` */
    COEF *coef;     /* host block, as the coefficients it holds */
    int mode;
};
template <int BD>
static void run_idct(uint8_t *dst, int stride, const BlockReq<Coef<BD>> *req, int n, int size)
{
    using PX = Px<BD>;
    using COEF = Coef<BD>;
    constexpr int B = sizeof(PX);
    if (!n) return;
    Arena &a = arena();
    int minx = 1 << 30, miny = 1 << 30, maxx = -(1 << 30), maxy = -(1 << 30);
    int bx[16], by[16];
    for (int i = 0; i < n; i++) {
        /* offsets are B * 4 * x + 4 * y * stride bytes with small x, y (h264_slice.c:485-494): recover samples and rows */
        const int y = req[i].off >= 0 ? (req[i].off + stride / 2) / stride : -((-req[i].off + stride / 2) / stride);
        const int x = (req[i].off - y * stride) / B;
        bx[i] = x; by[i] = y;
        if (x < minx) minx = x;
        if (y < miny) miny = y;
        if (x + size > maxx) maxx = x + size;
        if (y + size > maxy) maxy = y + size;
    }
    Win w = win_pack(a, dst + miny * (ptrdiff_t)stride + minx * B, stride, (maxx - minx) * B, maxy - miny);
    const size_t joff = a.take(sizeof(IdctJob<COEF>));
    IdctJob<COEF> *job = a.h<IdctJob<COEF>>(joff);
    std::memset(job, 0, sizeof(*job));
    job->n = n; job->size = size;
    for (int i = 0; i < n; i++) {
        std::memcpy(job->coef + i * size * size, req[i].coef, (size_t)size * size * sizeof(COEF));
        job->mode[i] = (uint8_t)req[i].mode;
        job->bx[i] = (uint8_t)(bx[i] - minx);
        job->by[i] = (uint8_t)(by[i] - miny);
    }
    a.upload();
    if constexpr (BD != 8) LAUNCH1(k_hbd_idct, a, a.d<PX>(w.off), w.pitch / B, a.d<IdctJob<COEF>>(joff), Smp<BD>::MAXV);
    else if (size == 4) LAUNCH1(k_idct4, a, a.d<PX>(w.off), w.pitch, a.d<IdctJob<COEF>>(joff));
    else LAUNCH1(k_idct8, a, a.d<PX>(w.off), w.pitch, a.d<IdctJob<COEF>>(joff));
    a.download();
    for (int i = 0; i < n; i++) {
        if (!req[i].mode) continue;
        win_unpack(a, w, dst + by[i] * (ptrdiff_t)stride + bx[i] * B, stride, (bx[i] - minx) * B, by[i] - miny, size * B, size);
        if (req[i].mode == 2) std::memset(req[i].coef, 0, (size_t)size * size * sizeof(COEF));
        else req[i].coef[0] = 0;
    }
}

static int scan8(int i)
{
    int p = i >> 4, b = i & 15;
    int x = (b & 1) + 2 * ((b >> 2) & 1), y = ((b >> 1) & 1) + 2 * (b >> 3);
    return 4 + x + 8 * (1 + y + 5 * p);
}
template <int BD> static Coef<BD> *co(int16_t *block, int i) { return reinterpret_cast<Coef<BD> *>(block) + i * 16; }      /* block i of a macroblock */

/* the four single-block entries: MODE 2 = full, 1 = dc only */
template <int SIZE, int MODE, int BD> static void idct_one_shim(uint8_t *dst, int16_t *block, int stride)
{
    BlockReq<Coef<BD>> r{0, co<BD>(block, 0), MODE};
    run_idct<BD>(dst, stride, &r, 1, SIZE);
}

/* dispatch rules of h264idct_template.c:174-214 */
template <int BD> static void t1_idct_add16(uint8_t *dst, const int *off, int16_t *block, int stride, const uint8_t nnzc[15 * 8])
{
    BlockReq<Coef<BD>> r[16]; int n = 0;
    for (int i = 0; i < 16; i++) {
        int nnz = nnzc[scan8(i)];
        if (nnz) r[n++] = {off[i], co<BD>(block, i), (nnz == 1 && co<BD>(block, i)[0]) ? 1 : 2};
    }
    run_idct<BD>(dst, stride, r, n, 4);
}
template <int BD> static void t1_idct_add16intra(uint8_t *dst, const int *off, int16_t *block, int stride, const uint8_t nnzc[15 * 8])
{
    BlockReq<Coef<BD>> r[16]; int n = 0;
    for (int i = 0; i < 16; i++) {
        if (nnzc[scan8(i)]) r[n++] = {off[i], co<BD>(block, i), 2};
        else if (co<BD>(block, i)[0]) r[n++] = {off[i], co<BD>(block, i), 1};
    }
    run_idct<BD>(dst, stride, r, n, 4);
}
template <int BD> static void t1_idct8_add4(uint8_t *dst, const int *off, int16_t *block, int stride, const uint8_t nnzc[15 * 8])
{
    BlockReq<Coef<BD>> r[4]; int n = 0;
    for (int i = 0; i < 16; i += 4) {
        int nnz = nnzc[scan8(i)];
        if (nnz) r[n++] = {off[i], co<BD>(block, i), (nnz == 1 && co<BD>(block, i)[0]) ? 1 : 2};
    }
    run_idct<BD>(dst, stride, r, n, 8);
}
template <int BD> static void t1_idct_add8(uint8_t **dest, const int *off, int16_t *block, int stride, const uint8_t nnzc[15 * 8])
{
    for (int j = 1; j < 3; j++) {
        BlockReq<Coef<BD>> r[4]; int n = 0;
        for (int i = j * 16; i < j * 16 + 4; i++) {
            if (nnzc[scan8(i)]) r[n++] = {off[i], co<BD>(block, i), 2};
            else if (co<BD>(block, i)[0]) r[n++] = {off[i], co<BD>(block, i), 1};
        }
        run_idct<BD>(dest[j - 1], stride, r, n, 4);
    }
}

/* ff_h264_idct_add8_422 h264idct_template.c:216-238: the second four blocks of a plane sit at block_offset[i + 4]
 * and are counted at scan8[i + 4] */
template <int BD> static void t1_idct_add8_422(uint8_t **dest, const int *off, int16_t *block, int stride, const uint8_t nnzc[15 * 8])
{
    for (int j = 1; j < 3; j++) {
        BlockReq<Coef<BD>> r[8]; int n = 0;
        for (int i = j * 16; i < j * 16 + 8; i++) {
            const int k = i < j * 16 + 4 ? i : i + 4;
            if (nnzc[scan8(k)]) r[n++] = {off[k], co<BD>(block, i), 2};
            else if (co<BD>(block, i)[0]) r[n++] = {off[k], co<BD>(block, i), 1};
        }
        run_idct<BD>(dest[j - 1], stride, r, n, 4);
    }
}

/* DC transforms :240-324 */
__global__ void __launch_bounds__(64) k_luma_dc(int16_t *out, const int16_t *in, int qmul)
{
    if (lane_id() == 0) {
        int v[16], o[16];
        for (int i = 0; i < 16; i++) v[i] = in[i];
        luma_dc_dequant(v, qmul, o);
        for (int k = 0; k < 16; k++) out[k] = (int16_t)o[k];
    }
}
__global__ void __launch_bounds__(64) k_chroma_dc(int16_t *v, int qmul)
{
    if (lane_id() == 0) {
        int a = v[0], b = v[1], c = v[2], d = v[3];
        chroma_dc_dequant(a, b, c, d, qmul);
        v[0] = (int16_t)a; v[1] = (int16_t)b; v[2] = (int16_t)c; v[3] = (int16_t)d;
    }
}
/* ff_h264_chroma422_dc_dequant_idct h264idct_template.c:277-303: 2x4 Hadamard of the eight DC levels
 * (block[32 * i + 16 * {0,1}]), (x * qmul + 128) >> 8, written back in place */
template <typename COEF> __device__ inline void chroma422_dc(COEF *v, int qmul)
{
    int t[8];
    for (int i = 0; i < 4; i++) { t[2 * i] = v[2 * i] + v[2 * i + 1]; t[2 * i + 1] = v[2 * i] - v[2 * i + 1]; }
    for (int i = 0; i < 2; i++) {
        const int z0 = t[i] + t[4 + i], z1 = t[i] - t[4 + i], z2 = t[2 + i] - t[6 + i], z3 = t[2 + i] + t[6 + i];
        v[0 + i] = (COEF)(((z0 + z3) * qmul + 128) >> 8);
        v[2 + i] = (COEF)(((z1 + z2) * qmul + 128) >> 8);
        v[4 + i] = (COEF)(((z1 - z2) * qmul + 128) >> 8);
        v[6 + i] = (COEF)(((z0 - z3) * qmul + 128) >> 8);
    }
}
__global__ void __launch_bounds__(64) k_chroma422_dc(int16_t *v, int qmul)
{
    if (lane_id() == 0) chroma422_dc(v, qmul);
}
/* 32-bit in and out, element positions as in the 8-bit kernels */
__global__ void __launch_bounds__(64) k_hbd_dc(int32_t *v, int qmul, int kind)
{
    if (lane_id() != 0) return;
    if (kind == 0) {                    /* luma: 16 values in, luma_dc_dequant order out */
        /* the butterflies of luma_dc_dequant (h264_dev.h) without its 16-bit store: dctcoef is 32 bits wide here */
        int t[16];
        for (int i = 0; i < 4; i++) {
            const int s = v[4 * i] + v[4 * i + 1], d = v[4 * i] - v[4 * i + 1];
            const int e = v[4 * i + 2] - v[4 * i + 3], u = v[4 * i + 2] + v[4 * i + 3];
            t[4 * i] = s + u; t[4 * i + 1] = s - u; t[4 * i + 2] = d - e; t[4 * i + 3] = d + e;
        }
        for (int i = 0; i < 4; i++) {
            const int s = t[i] + t[8 + i], d = t[i] - t[8 + i];
            const int e = t[4 + i] - t[12 + i], u = t[4 + i] + t[12 + i];
            v[16 + 4 * i + 0] = ((s + u) * qmul + 128) >> 8;
            v[16 + 4 * i + 1] = ((d + e) * qmul + 128) >> 8;
            v[16 + 4 * i + 2] = ((d - e) * qmul + 128) >> 8;
            v[16 + 4 * i + 3] = ((s - u) * qmul + 128) >> 8;
        }
    } else if (kind == 1) {             /* chroma 4:2:0, :312-324 */
        const int a = v[0], b = v[1], c = v[2], d = v[3];
        const int s0 = a + b, d0 = a - b, s1 = c + d, d1 = c - d;
        v[0] = ((s0 + s1) * qmul) >> 7; v[1] = ((d0 + d1) * qmul) >> 7; v[2] = ((s0 - s1) * qmul) >> 7; v[3] = ((d0 - d1) * qmul) >> 7;
    } else chroma422_dc(v, qmul);       /* chroma 4:2:2, :275-310 */
}
/* the three shims stage 16 + 16 (in, out), 4 or 8 levels; kind as k_hbd_dc's */
template <int BD> static void launch_dc(Arena &a, size_t off, int qmul, int kind)
{
    Coef<BD> *v = a.d<Coef<BD>>(off);
    if constexpr (BD != 8) LAUNCH1(k_hbd_dc, a, v, qmul, kind);
    else if (kind == 0) LAUNCH1(k_luma_dc, a, v + 16, v, qmul);
    else if (kind == 1) LAUNCH1(k_chroma_dc, a, v, qmul);
    else LAUNCH1(k_chroma422_dc, a, v, qmul);
}
template <int BD> static void t1_luma_dc_dequant_idct(int16_t *output, int16_t *input, int qmul)
{
    using COEF = Coef<BD>;
    Arena &a = arena();
    const size_t off = a.take(32 * sizeof(COEF));
    COEF *h = a.h<COEF>(off);
    std::memcpy(h, input, 16 * sizeof(COEF));
    a.upload();
    launch_dc<BD>(a, off, qmul, 0);
    a.download();
    for (int k = 0; k < 16; k++) reinterpret_cast<COEF *>(output)[luma_dc_slot(k)] = h[16 + k];
}
template <int BD> static void t1_chroma_dc_dequant_idct(int16_t *block16, int qmul)
{
    Coef<BD> *block = reinterpret_cast<Coef<BD> *>(block16);
    Arena &a = arena();
    const size_t off = a.take(4 * sizeof(Coef<BD>));
    Coef<BD> *h = a.h<Coef<BD>>(off);
    for (int k = 0; k < 4; k++) h[k] = block[16 * k];
    a.upload();
    launch_dc<BD>(a, off, qmul, 1);
    a.download();
    for (int k = 0; k < 4; k++) block[16 * k] = h[k];
}
template <int BD> static void t1_chroma422_dc_dequant_idct(int16_t *block16, int qmul)
{
    Coef<BD> *block = reinterpret_cast<Coef<BD> *>(block16);
    Arena &a = arena();
    const size_t off = a.take(8 * sizeof(Coef<BD>));
    Coef<BD> *h = a.h<Coef<BD>>(off);
    for (int i = 0; i < 4; i++) { h[2 * i] = block[32 * i]; h[2 * i + 1] = block[32 * i + 16]; }
    a.upload();
    launch_dc<BD>(a, off, qmul, 2);
    a.download();
    /* output k of row i lands at block[32 * i + {0, 16}] (x_offset[] = {0, 16}, stride 32) */
    for (int i = 0; i < 4; i++) { block[32 * i] = h[2 * i]; block[32 * i + 16] = h[2 * i + 1]; }
}

/* ------------------------------------------------------------------------- */
/* weighted prediction: h264dsp_template.c:30-98                               */
/* ------------------------------------------------------------------------- */
__global__ void __launch_bounds__(64)
k_weight(uint8_t *p, int pitch, int w, int h, int ld, int wt, int off)
{
    weight_block(p, pitch, w, h, ld, wt, off);
}
__global__ void __launch_bounds__(64)
k_biweight(uint8_t *d, const uint8_t *s, int pitch, int w, int h, int ld, int wd, int ws, int off)
{
    biweight_block(d, s, pitch, w, h, ld, wd, ws, off);
}
__global__ void __launch_bounds__(64)
k_hbd_weight(uint16_t *p, int pitch, int w, int h, int ld, int wt, int off, int bd)
{
    int o = (int)((unsigned)off << (ld + (bd - 8)));
    if (ld) o += 1 << (ld - 1);
    for (int i = lane_id(); i < w * h; i += 64) {
        const int y = i / w, x = i - y * w;
        p[y * pitch + x] = (uint16_t)clip3((p[y * pitch + x] * wt + o) >> ld, 0, (1 << bd) - 1);
    }
}
__global__ void __launch_bounds__(64)
k_hbd_biweight(uint16_t *d, const uint16_t *s, int pitch, int w, int h, int ld, int wd, int ws, int off, int bd)
{
    const int o = (int)((unsigned)((((int)((unsigned)off << (bd - 8))) + 1) | 1) << ld);
    for (int i = lane_id(); i < w * h; i += 64) {
        const int y = i / w, x = i - y * w;
        d[y * pitch + x] = (uint16_t)clip3((s[y * pitch + x] * ws + d[y * pitch + x] * wd + o) >> (ld + 1), 0, (1 << bd) - 1);
    }
}
template <int W, int BD>
static void weight_shim(uint8_t *block, int stride, int height, int log2_denom, int weight, int offset)
{
    using PX = Px<BD>;
    constexpr int B = sizeof(PX);
    Arena &a = arena();
    Win w = win_pack(a, block, stride, W * B, height);
    a.upload();
    if constexpr (BD == 8) LAUNCH1(k_weight, a, a.d<PX>(w.off), w.pitch, W, height, log2_denom, weight, offset);
    else LAUNCH1(k_hbd_weight, a, a.d<PX>(w.off), w.pitch / B, W, height, log2_denom, weight, offset, BD);
    a.download();
    win_unpack(a, w, block, stride, 0, 0, W * B, height);
}
template <int W, int BD>
static void biweight_shim(uint8_t *dst, uint8_t *src, int stride, int height, int log2_denom,
                          int weightd, int weights, int offset)
{
    using PX = Px<BD>;
    constexpr int B = sizeof(PX);
    Arena &a = arena();
    Win d = win_pack(a, dst, stride, W * B, height);
    Win s = win_pack(a, src, stride, W * B, height);
    a.upload();
    if constexpr (BD == 8) LAUNCH1(k_biweight, a, a.d<PX>(d.off), a.d<PX>(s.off), d.pitch, W, height, log2_denom, weightd, weights, offset);
    else LAUNCH1(k_hbd_biweight, a, a.d<PX>(d.off), a.d<PX>(s.off), d.pitch / B, W, height, log2_denom, weightd, weights, offset, BD);
    a.download();
    win_unpack(a, d, dst, stride, 0, 0, W * B, height);
}

/* ------------------------------------------------------------------------- */
/* deblocking edge filters: h264dsp_template.c:104-330                         */
/* ------------------------------------------------------------------------- */
/* window sample (across index k in [-R,R), line n) = win[(k+R)*xs + n*ys], strides in samples */
struct LfJob {
    int xs, ys, nlines, inner, alpha, beta, kind; /* kind: 0 luma, 1 luma intra, 2 chroma, 3 chroma intra */
    int R;
    int tc[4];                                    /* alpha, beta and tc already scaled for the bit depth */
};
template <int BD>
__global__ void __launch_bounds__(64) k_loopfilter(Px<BD> *win, const LfJob *jp)
{
    using PX = Px<BD>;
    constexpr int MAXV = Smp<BD>::MAXV;
    const LfJob j = *jp;
    const int n = lane_id();
    if (n >= j.nlines) return;
    PX *c = win + j.R * j.xs + n * j.ys; /* q0 */
#define AT(k) c[(k) * j.xs]
    if (j.kind == 0) {
        int p2 = AT(-3), p1 = AT(-2), p0 = AT(-1), q0 = AT(0), q1 = AT(1), q2 = AT(2);
        lf_luma_line<MAXV>(p2, p1, p0, q0, q1, q2, j.alpha, j.beta, j.tc[n / j.inner]);
        AT(-2) = (PX)p1; AT(-1) = (PX)p0; AT(0) = (PX)q0; AT(1) = (PX)q1;
    } else if (j.kind == 1) {
        int p3 = AT(-4), p2 = AT(-3), p1 = AT(-2), p0 = AT(-1), q0 = AT(0), q1 = AT(1), q2 = AT(2), q3 = AT(3);
        lf_luma_intra_line(p3, p2, p1, p0, q0, q1, q2, q3, j.alpha, j.beta);
        AT(-3) = (PX)p2; AT(-2) = (PX)p1; AT(-1) = (PX)p0;
        AT(0) = (PX)q0; AT(1) = (PX)q1; AT(2) = (PX)q2;
    } else {
        int p1 = AT(-2), p0 = AT(-1), q0 = AT(0), q1 = AT(1);
        if (j.kind == 2) lf_chroma_line<MAXV>(p1, p0, q0, q1, j.alpha, j.beta, j.tc[n / j.inner]);
        else lf_chroma_intra_line(p1, p0, q0, q1, j.alpha, j.beta);
        AT(-1) = (PX)p0; AT(0) = (PX)q0;
    }
#undef AT
}
/* vertical_edge: samples across the edge are adjacent in memory ("h_loop_filter") */
template <int BD>
static void lf_shim(uint8_t *pix, int stride, int alpha, int beta, const int8_t *tc0, int kind, int vertical_edge, int inner)
{
    using PX = Px<BD>;
    constexpr int B = sizeof(PX);
    Arena &a = arena();
    const int R = kind == 1 ? 4 : (kind == 0 ? 3 : 2), W = kind <= 1 ? 3 : 1;
    const int nlines = 4 * inner;
    Win w = vertical_edge ? win_pack(a, pix - R * B, stride, 2 * R * B, nlines)
                          : win_pack(a, pix - R * (ptrdiff_t)stride, stride, nlines * B, 2 * R);
    size_t joff = a.take(sizeof(LfJob));
    LfJob *j = a.h<LfJob>(joff);
    j->xs = vertical_edge ? 1 : w.pitch / B;
    j->ys = vertical_edge ? w.pitch / B : 1;
    j->nlines = nlines; j->inner = inner; j->kind = kind; j->R = R;
    j->alpha = alpha << (BD - 8); j->beta = beta << (BD - 8);               /* :110-111 */
    for (int i = 0; i < 4; i++) {
        const int t = tc0 ? tc0[i] : 0;
        j->tc[i] = kind == 0 ? t * (1 << (BD - 8)) : (t - 1) * (1 << (BD - 8)) + 1;      /* :113, :228 */
    }
    a.upload();
    LAUNCH1(k_loopfilter<BD>, a, a.d<PX>(w.off), a.d<LfJob>(joff));
    a.download();
    if (vertical_edge) win_unpack(a, w, pix - W * B, stride, (R - W) * B, 0, 2 * W * B, nlines);
    else               win_unpack(a, w, pix - W * (ptrdiff_t)stride, stride, 0, R - W, nlines * B, 2 * W);
}
#define LF_TC(name, kind, vert, inner) \
    template <int BD> static void name(uint8_t *pix, int stride, int alpha, int beta, int8_t *tc0) { lf_shim<BD>(pix, stride, alpha, beta, tc0, kind, vert, inner); }
#define LF_IN(name, kind, vert, inner) \
    template <int BD> static void name(uint8_t *pix, int stride, int alpha, int beta) { lf_shim<BD>(pix, stride, alpha, beta, nullptr, kind, vert, inner); }
LF_TC(t1_v_lf_luma, 0, 0, 4) LF_TC(t1_h_lf_luma, 0, 1, 4) LF_TC(t1_h_lf_luma_mbaff, 0, 1, 2)
LF_IN(t1_v_lf_luma_intra, 1, 0, 4) LF_IN(t1_h_lf_luma_intra, 1, 1, 4) LF_IN(t1_h_lf_luma_mbaff_intra, 1, 1, 2)
LF_TC(t1_v_lf_chroma, 2, 0, 2) LF_TC(t1_h_lf_chroma, 2, 1, 2) LF_TC(t1_h_lf_chroma_mbaff, 2, 1, 1)
LF_IN(t1_v_lf_chroma_intra, 3, 0, 2) LF_IN(t1_h_lf_chroma_intra, 3, 1, 2) LF_IN(t1_h_lf_chroma_mbaff_intra, 3, 1, 1)
/* 4:2:2: the chroma edge of a macroblock is 16 lines high (h264dsp_template.c:276-283, :321-328) */
LF_TC(t1_h_lf_chroma422, 2, 1, 4) LF_TC(t1_h_lf_chroma422_mbaff, 2, 1, 2)
LF_IN(t1_h_lf_chroma422_intra, 3, 1, 4) LF_IN(t1_h_lf_chroma422_mbaff_intra, 3, 1, 2)
#undef LF_TC
#undef LF_IN

/* ---- a4: transform-bypass residual add, h264addpx_template.c:30-72: dst += residual without
 * clipping (wraps like the reference's pixel type, 8 or 16 bits, not at the bit depth), block cleared afterwards -- */
template <typename PX>
__global__ void __launch_bounds__(64) k_add_pixels(PX *dst, int pitch, const CoefOf<PX> *blk, int n)
{
    for (int i = lane_id(); i < n * n; i += 64) {
        const int y = i / n, x = i - y * n;
        dst[y * pitch + x] = (PX)(dst[y * pitch + x] + blk[i]);
    }
}
template <int N, int BD> static void add_pixels_clear_shim(uint8_t *dst, int16_t *block, int stride)
{
    using PX = Px<BD>;
    using COEF = Coef<BD>;
    constexpr int B = sizeof(PX);
    Arena &a = arena();
    Win w = win_pack(a, dst, stride, N * B, N);
    const size_t b = a.take(N * N * sizeof(COEF));
    std::memcpy(a.h<COEF>(b), block, N * N * sizeof(COEF));
    a.upload();
    LAUNCH1(k_add_pixels<PX>, a, a.d<PX>(w.off), w.pitch / B, a.d<const COEF>(b), N);
    a.download();
    win_unpack(a, w, dst, stride, 0, 0, N * B, N);
    std::memset(block, 0, N * N * sizeof(COEF));
}

template <int BD> static void fill_dsp(H264DSPContext *c, int chroma_format_idc)
{
    /* like an arch hook: only the variants this backend implements are overridden
     * (4:0:0, 4:2:0 and 4:2:2 — 4:4:4 chroma goes through the luma entries); everything else keeps the C default */
    c->weight_h264_pixels_tab[0] = weight_shim<16, BD>;   c->weight_h264_pixels_tab[1] = weight_shim<8, BD>;
    c->weight_h264_pixels_tab[2] = weight_shim<4, BD>;    c->weight_h264_pixels_tab[3] = weight_shim<2, BD>;
    c->biweight_h264_pixels_tab[0] = biweight_shim<16, BD>; c->biweight_h264_pixels_tab[1] = biweight_shim<8, BD>;
    c->biweight_h264_pixels_tab[2] = biweight_shim<4, BD>;  c->biweight_h264_pixels_tab[3] = biweight_shim<2, BD>;
    c->h264_v_loop_filter_luma = t1_v_lf_luma<BD>;
    c->h264_h_loop_filter_luma = t1_h_lf_luma<BD>;
    c->h264_h_loop_filter_luma_mbaff = t1_h_lf_luma_mbaff<BD>;
    c->h264_v_loop_filter_luma_intra = t1_v_lf_luma_intra<BD>;
    c->h264_h_loop_filter_luma_intra = t1_h_lf_luma_intra<BD>;
    c->h264_h_loop_filter_luma_mbaff_intra = t1_h_lf_luma_mbaff_intra<BD>;
    c->h264_v_loop_filter_chroma = t1_v_lf_chroma<BD>;
    c->h264_v_loop_filter_chroma_intra = t1_v_lf_chroma_intra<BD>;
    c->h264_idct_add = idct_one_shim<4, 2, BD>;
    c->h264_idct8_add = idct_one_shim<8, 2, BD>;
    c->h264_idct_dc_add = idct_one_shim<4, 1, BD>;
    c->h264_idct8_dc_add = idct_one_shim<8, 1, BD>;
    c->h264_idct_add16 = t1_idct_add16<BD>;
    c->h264_idct8_add4 = t1_idct8_add4<BD>;
    c->h264_idct_add16intra = t1_idct_add16intra<BD>;
    c->h264_luma_dc_dequant_idct = t1_luma_dc_dequant_idct<BD>;
    c->h264_add_pixels4_clear = add_pixels_clear_shim<4, BD>;
    c->h264_add_pixels8_clear = add_pixels_clear_shim<8, BD>;
    if (chroma_format_idc <= 1) {
        c->h264_h_loop_filter_chroma = t1_h_lf_chroma<BD>;
        c->h264_h_loop_filter_chroma_mbaff = t1_h_lf_chroma_mbaff<BD>;
        c->h264_h_loop_filter_chroma_intra = t1_h_lf_chroma_intra<BD>;
        c->h264_h_loop_filter_chroma_mbaff_intra = t1_h_lf_chroma_mbaff_intra<BD>;
        c->h264_idct_add8 = t1_idct_add8<BD>;
        c->h264_chroma_dc_dequant_idct = t1_chroma_dc_dequant_idct<BD>;
    } else {   /* 4:2:2, and 4:4:4 like the reference (h264dsp.c:80-130: every idc > 1 gets the 4:2:2 forms; 4:4:4 decoding does not call them) */
        c->h264_h_loop_filter_chroma = t1_h_lf_chroma422<BD>;
        c->h264_h_loop_filter_chroma_mbaff = t1_h_lf_chroma422_mbaff<BD>;
        c->h264_h_loop_filter_chroma_intra = t1_h_lf_chroma422_intra<BD>;
        c->h264_h_loop_filter_chroma_mbaff_intra = t1_h_lf_chroma422_mbaff_intra<BD>;
        c->h264_idct_add8 = t1_idct_add8_422<BD>;
        c->h264_chroma_dc_dequant_idct = t1_chroma422_dc_dequant_idct<BD>;
    }
}
/* the hooks serve bit depths 8, 9 and 10; any other depth keeps the C default */
void ff_h264dsp_init_mi355x(H264DSPContext *c, const int bit_depth, const int chroma_format_idc)
{
    if (bit_depth == 8) fill_dsp<8>(c, chroma_format_idc);
    else if (bit_depth == 9) fill_dsp<9>(c, chroma_format_idc);
    else if (bit_depth == 10) fill_dsp<10>(c, chroma_format_idc);
}

template <int BD> static void fill_qpel(H264QpelContext *c)
{
#define QROW(tab, idx, SIZE, AVG) \
    c->tab[idx][0] = qpel_shim<SIZE, 0, AVG, BD>;   c->tab[idx][1] = qpel_shim<SIZE, 1, AVG, BD>;   \
    c->tab[idx][2] = qpel_shim<SIZE, 2, AVG, BD>;   c->tab[idx][3] = qpel_shim<SIZE, 3, AVG, BD>;   \
    c->tab[idx][4] = qpel_shim<SIZE, 4, AVG, BD>;   c->tab[idx][5] = qpel_shim<SIZE, 5, AVG, BD>;   \
    c->tab[idx][6] = qpel_shim<SIZE, 6, AVG, BD>;   c->tab[idx][7] = qpel_shim<SIZE, 7, AVG, BD>;   \
    c->tab[idx][8] = qpel_shim<SIZE, 8, AVG, BD>;   c->tab[idx][9] = qpel_shim<SIZE, 9, AVG, BD>;   \
    c->tab[idx][10] = qpel_shim<SIZE, 10, AVG, BD>; c->tab[idx][11] = qpel_shim<SIZE, 11, AVG, BD>; \
    c->tab[idx][12] = qpel_shim<SIZE, 12, AVG, BD>; c->tab[idx][13] = qpel_shim<SIZE, 13, AVG, BD>; \
    c->tab[idx][14] = qpel_shim<SIZE, 14, AVG, BD>; c->tab[idx][15] = qpel_shim<SIZE, 15, AVG, BD>;
    QROW(put_h264_qpel_pixels_tab, 0, 16, 0) QROW(put_h264_qpel_pixels_tab, 1, 8, 0)
    QROW(put_h264_qpel_pixels_tab, 2, 4, 0)  QROW(put_h264_qpel_pixels_tab, 3, 2, 0)
    QROW(avg_h264_qpel_pixels_tab, 0, 16, 1) QROW(avg_h264_qpel_pixels_tab, 1, 8, 1)
    QROW(avg_h264_qpel_pixels_tab, 2, 4, 1)
#undef QROW
}
void ff_h264qpel_init_mi355x(H264QpelContext *c, int bit_depth)
{
    if (bit_depth == 8) fill_qpel<8>(c);
    else if (bit_depth == 9) fill_qpel<9>(c);
    else if (bit_depth == 10) fill_qpel<10>(c);
}

template <int BD> static void fill_chroma(H264ChromaContext *c)
{
    c->put_h264_chroma_pixels_tab[0] = chroma_shim<8, 0, BD>; c->put_h264_chroma_pixels_tab[1] = chroma_shim<4, 0, BD>;
    c->put_h264_chroma_pixels_tab[2] = chroma_shim<2, 0, BD>;
    c->avg_h264_chroma_pixels_tab[0] = chroma_shim<8, 1, BD>; c->avg_h264_chroma_pixels_tab[1] = chroma_shim<4, 1, BD>;
    c->avg_h264_chroma_pixels_tab[2] = chroma_shim<2, 1, BD>;
}
void ff_h264chroma_init_mi355x(H264ChromaContext *c, int bit_depth)
{
    if (bit_depth == 8) fill_chroma<8>(c);
    else if (bit_depth == 9) fill_chroma<9>(c);
    else if (bit_depth == 10) fill_chroma<10>(c);
}

/* ------------------------------------------------------------------------- */
/* intra prediction: h264pred_template.c, the predictors of h264_dev.h         */
/* ------------------------------------------------------------------------- */
struct PredJob {
    uint16_t T[1 + 32], L[1 + 16];      /* 16-bit at every depth, like PredScratch */
    int kind, mode, has_tl, has_tr;
};
template <int BD>
__global__ void __launch_bounds__(64) k_pred(const PredJob *jp, Px<BD> *out, int pitch)
{
    __shared__ PredScratch s;
    const int lane = lane_id();
    if (lane < 33) s.T[lane] = jp->T[lane];
    if (lane < 17) s.L[lane] = jp->L[lane];
    __syncthreads();
    intra_pred_wave<Px<BD>, BD>(s, jp->kind, jp->mode, jp->has_tl, jp->has_tr, out, pitch);
}

/* gather only the edge samples the reference reads for this (kind, mode, availability) */
template <int BD>
static void pred_shim(uint8_t *src8, ptrdiff_t stride, int kind, int mode, int has_tl, int has_tr, const uint8_t *topright8)
{
    using PX = Px<BD>;
    constexpr int B = sizeof(PX);
    Arena &a = arena();
    const PX *src = reinterpret_cast<const PX *>(src8), *topright = reinterpret_cast<const PX *>(topright8);
    const ptrdiff_t st = stride / B;
    const int N = kind == 0 ? 4 : (kind == 3 ? 16 : 8);          /* width */
    const int NH = kind == 4 ? 16 : N;                              /* height: 8x16 for 4:2:2 chroma */
    size_t joff = a.take(sizeof(PredJob));
    PredJob *j = a.h<PredJob>(joff);
    std::memset(j, 0, sizeof(*j));
    j->kind = kind; j->mode = mode; j->has_tl = has_tl; j->has_tr = has_tr;
    int top = 0, left = 0, corner = 0, tr = 0;
    if (kind <= 1) {
        int needs = pred_luma_needs(mode);
        top = needs & 1; left = (needs >> 1) & 1; corner = (needs >> 2) & 1; tr = (needs >> 3) & 1;
        if (kind == 1) {
            if ((top || left) && has_tl) corner = 1;
            if (top && has_tr) tr = 1;          /* t7's filter reads p[8,-1] */
            if (tr && !has_tr) tr = 0;
        }
    } else if (kind == 3) {
        top = mode == 0 || mode == 2 || mode == 3 || mode == 5;
        left = mode == 0 || mode == 1 || mode == 3 || mode == 4;
        corner = mode == 3;
    } else {
        top = mode == 0 || mode == 2 || mode == 3 || mode == 5 || mode == 7 || mode == 8;
        left = mode == 0 || mode == 1 || mode == 3 || mode == 4 || mode >= 7;
        corner = mode == 3;
    }
    if (top) for (int i = 0; i < N; i++) j->T[1 + i] = src[i - st];
    if (left) for (int i = 0; i < NH; i++) j->L[1 + i] = src[-1 + i * st];
    if (corner) j->T[0] = j->L[0] = src[-1 - st];
    if (tr) {
        if (kind == 0) for (int i = 0; i < 4; i++) j->T[5 + i] = topright[i];
        else for (int i = 0; i < 8; i++) j->T[9 + i] = src[8 + i - st];
    }
    size_t ooff = a.take((size_t)NH * 16 * B);
    a.upload();
    LAUNCH1(k_pred<BD>, a, a.d<PredJob>(joff), a.d<PX>(ooff), 16);
    a.download();
    const uint8_t *o = a.h<uint8_t>(ooff);
    for (int y = 0; y < NH; y++) std::memcpy(src8 + y * stride, o + y * 16 * B, (size_t)N * B);
}
template <int M, int BD> static void p4_shim(uint8_t *s, const uint8_t *tr, ptrdiff_t st) { pred_shim<BD>(s, st, 0, M, 0, 1, tr); }
template <int M, int BD> static void p8l_shim(uint8_t *s, int tl, int tr, ptrdiff_t st) { pred_shim<BD>(s, st, 1, M, tl != 0, tr != 0, nullptr); }
template <int M, int BD> static void p8_shim(uint8_t *s, ptrdiff_t st) { pred_shim<BD>(s, st, 2, M, 0, 0, nullptr); }
template <int M, int BD> static void p16_shim(uint8_t *s, ptrdiff_t st) { pred_shim<BD>(s, st, 3, M, 0, 0, nullptr); }
template <int M, int BD> static void p8x16_shim(uint8_t *s, ptrdiff_t st) { pred_shim<BD>(s, st, 4, M, 0, 0, nullptr); }

/* ---- a10, lossless variants: prediction + residual as a running sum (h264pred_template.c:1127-1354) ----
 * Lane = (block, line); the sum starts at the neighbouring sample (or the (1,2,1)-filtered edge for the
 * 8x8 `filter_add` slots) and wraps at 8 or 16 bits at every step like the reference's pixel type (not at the
 * bit depth).  Blocks that feed each other (a block below / right of another one of the same call) run in rounds. */
template <typename COEF> struct PredAddJob {
    COEF coef[16 * 16];
    uint8_t bx[16], by[16];          /* block origin inside the window */
    int32_t n, size, horizontal, filtered, has_tl, has_tr;
};
template <typename PX>
__global__ void __launch_bounds__(64) k_pred_add(PX *win, int pitch, const PredAddJob<CoefOf<PX>> *job)
{
    const int lane = lane_id(), size = job->size, b = lane / size, i = lane - b * size;
    const bool mine = b < job->n;
    const int bx = mine ? job->bx[b] : 0, by = mine ? job->by[b] : 0, hz = job->horizontal;
#define AT(x, y) win[(by + (y)) * pitch + bx + (x)]
    for (int round = 0; round < 4; round++) {
        /* blocks whose origin along the prediction direction is `round` blocks from the window's first block */
        const int along = hz ? bx - 1 : by - 1;      /* the window starts one sample before the first block */
        if (mine && (job->filtered || (along >> 2) == round) && (!job->filtered || round == 0)) {
            int v;
            if (!job->filtered) v = hz ? AT(-1, i) : AT(i, -1);
            else if (!hz) {      /* PREDICT_8x8_LOAD_TOP :857-862 */
                const int c = AT(i, -1);
                const int lft = i == 0 ? (job->has_tl ? AT(-1, -1) : c) : AT(i - 1, -1);
                const int rgt = i == 7 ? (job->has_tr ? AT(8, -1) : c) : AT(i + 1, -1);
                v = (lft + 2 * c + rgt + 2) >> 2;
            } else {             /* PREDICT_8x8_LOAD_LEFT :849-853 */
                const int c = AT(-1, i);
                const int up = i == 0 ? (job->has_tl ? AT(-1, -1) : c) : AT(-1, i - 1);
                v = i == 7 ? (AT(-1, 6) + 3 * c + 2) >> 2 : (up + 2 * c + AT(-1, i + 1) + 2) >> 2;
            }
            const CoefOf<PX> *blk = job->coef + b * size * size;
            for (int k = 0; k < size; k++) {
                v = (PX)(v + (hz ? blk[i * size + k] : blk[k * size + i]));
                if (hz) AT(k, i) = (PX)v; else AT(i, k) = (PX)v;
            }
        }
        __syncthreads();
    }
#undef AT
}
template <int BD>
static void pred_add_run(uint8_t *pix, const int *offs, int nblk, int16_t *block, ptrdiff_t stride, int size, int horizontal,
                         int filtered, int has_tl, int has_tr)
{
    using PX = Px<BD>;
    using COEF = Coef<BD>;
    constexpr int B = sizeof(PX);
    Arena &a = arena();
    int bx[16], by[16], minx = 1 << 30, miny = 1 << 30, maxx = -(1 << 30), maxy = -(1 << 30);
    for (int i = 0; i < nblk; i++) {
        const int off = offs ? offs[i] : 0;
        const int y = off >= 0 ? (off + (int)stride / 2) / (int)stride : -((-off + (int)stride / 2) / (int)stride);
        bx[i] = (off - y * (int)stride) / B; by[i] = y;
        if (bx[i] < minx) minx = bx[i];
        if (by[i] < miny) miny = by[i];
        if (bx[i] + size > maxx) maxx = bx[i] + size;
        if (by[i] + size > maxy) maxy = by[i] + size;
    }
    /* exactly the samples the reference reads: one line before the blocks along the prediction direction,
     * and for the filtered 8x8 forms the corner / the sample past the edge only when the flags say so */
    const int x0 = horizontal ? minx - 1 : minx;                               /* the blocks' rows */
    int ax0 = minx, ax1 = maxx, y0 = miny - 1;                                 /* the row above them */
    if (filtered && !horizontal) { ax0 -= has_tl ? 1 : 0; ax1 += has_tr ? 1 : 0; }
    if (horizontal) { ax0 = minx - 1; ax1 = minx; y0 = miny - (filtered && has_tl ? 1 : 0); }
    /* the kernel addresses blocks relative to a window that starts one sample before them in both axes */
    const int wx0 = minx - 1, wy0 = miny - 1;
    Win w = win_pack(a, nullptr, 0, (maxx + 1 - wx0) * B, maxy - wy0, 0, 0);
    for (int y = y0; y < maxy; y++) {
        const int rx0 = y < miny ? ax0 : x0, rx1 = y < miny ? ax1 : maxx;
        std::memcpy(a.h<uint8_t>(w.off) + (size_t)(y - wy0) * w.pitch + (rx0 - wx0) * B, pix + y * stride + rx0 * B, (size_t)(rx1 - rx0) * B);
    }
    const size_t joff = a.take(sizeof(PredAddJob<COEF>));
    PredAddJob<COEF> *job = a.h<PredAddJob<COEF>>(joff);
    std::memset(job, 0, sizeof(*job));
    std::memcpy(job->coef, block, sizeof(COEF) * (size_t)nblk * size * size);
    for (int i = 0; i < nblk; i++) { job->bx[i] = (uint8_t)(bx[i] - wx0); job->by[i] = (uint8_t)(by[i] - wy0); }
    job->n = nblk; job->size = size; job->horizontal = horizontal; job->filtered = filtered; job->has_tl = has_tl; job->has_tr = has_tr;
    a.upload();
    LAUNCH1(k_pred_add<PX>, a, a.d<PX>(w.off), w.pitch / B, a.d<const PredAddJob<COEF>>(joff));
    a.download();
    for (int i = 0; i < nblk; i++)
        win_unpack(a, w, pix + by[i] * stride + bx[i] * B, stride, (bx[i] - wx0) * B, by[i] - wy0, size * B, size);
    std::memset(block, 0, sizeof(COEF) * (size_t)nblk * size * size);
}
template <int SIZE, int HZ, int BD> static void pred_add_shim(uint8_t *pix, int16_t *block, ptrdiff_t stride)
{
    pred_add_run<BD>(pix, nullptr, 1, block, stride, SIZE, HZ, 0, 0, 0);
}
template <int HZ, int BD> static void pred8x8l_filter_add_shim(uint8_t *pix, int16_t *block, int tl, int tr, ptrdiff_t stride)
{
    pred_add_run<BD>(pix, nullptr, 1, block, stride, 8, HZ, 1, tl != 0, tr != 0);
}
template <int NBLK, int HZ, int BD> static void pred_multi_add_shim(uint8_t *pix, const int *block_offset, int16_t *block, ptrdiff_t stride)
{
    pred_add_run<BD>(pix, block_offset, NBLK, block, stride, 4, HZ, 0, 0, 0);
}
/* pred8x16_{vertical,horizontal}_add :1326-1354: blocks 0..3 at block_offset[0..3], 4..7 at block_offset[8..11] */
template <int HZ, int BD> static void pred8x16_add_shim(uint8_t *pix, const int *block_offset, int16_t *block, ptrdiff_t stride)
{
    int offs[8];
    for (int i = 0; i < 4; i++) { offs[i] = block_offset[i]; offs[4 + i] = block_offset[8 + i]; }
    pred_add_run<BD>(pix, offs, 8, block, stride, 4, HZ, 0, 0, 0);
}

template <int BD> static void fill_pred(H264PredContext *h, int chroma_format_idc)
{
#define P11(tab, shim) \
    h->tab[0] = shim<0, BD>; h->tab[1] = shim<1, BD>; h->tab[2] = shim<2, BD>; h->tab[3] = shim<3, BD>; h->tab[4] = shim<4, BD>; h->tab[5] = shim<5, BD>; \
    h->tab[6] = shim<6, BD>; h->tab[7] = shim<7, BD>; h->tab[8] = shim<8, BD>; h->tab[9] = shim<9, BD>; h->tab[10] = shim<10, BD>;
    P11(pred4x4, p4_shim)   h->pred4x4[11] = p4_shim<11, BD>;
    P11(pred8x8l, p8l_shim) h->pred8x8l[11] = p8l_shim<11, BD>;
    if (chroma_format_idc <= 1) { P11(pred8x8, p8_shim) }
    else { P11(pred8x8, p8x16_shim) }   /* idc > 1: the same slots hold the 8x16 predictors, as h264pred.c:470-565 selects them */
#undef P11
    h->pred16x16[0] = p16_shim<0, BD>; h->pred16x16[1] = p16_shim<1, BD>; h->pred16x16[2] = p16_shim<2, BD>; h->pred16x16[3] = p16_shim<3, BD>;
    h->pred16x16[4] = p16_shim<4, BD>; h->pred16x16[5] = p16_shim<5, BD>; h->pred16x16[6] = p16_shim<6, BD>;
    /* lossless (transform bypass) forms: VERT_PRED 0 / HOR_PRED 1; VERT_PRED8x8 2 / HOR_PRED8x8 1 (h264pred.c:551-565) */
    h->pred4x4_add[0] = pred_add_shim<4, 0, BD>;   h->pred4x4_add[1] = pred_add_shim<4, 1, BD>;
    h->pred8x8l_add[0] = pred_add_shim<8, 0, BD>;  h->pred8x8l_add[1] = pred_add_shim<8, 1, BD>;
    h->pred8x8l_filter_add[0] = pred8x8l_filter_add_shim<0, BD>; h->pred8x8l_filter_add[1] = pred8x8l_filter_add_shim<1, BD>;
    if (chroma_format_idc <= 1) { h->pred8x8_add[2] = pred_multi_add_shim<4, 0, BD>; h->pred8x8_add[1] = pred_multi_add_shim<4, 1, BD>; }
    else { h->pred8x8_add[2] = pred8x16_add_shim<0, BD>; h->pred8x8_add[1] = pred8x16_add_shim<1, BD>; }
    h->pred16x16_add[2] = pred_multi_add_shim<16, 0, BD>; h->pred16x16_add[1] = pred_multi_add_shim<16, 1, BD>;
}
void ff_h264_pred_init_mi355x(H264PredContext *h, int codec_id, const int bit_depth, const int chroma_format_idc)
{
    if (codec_id != MI355_AV_CODEC_ID_H264) return;
    if (bit_depth == 8) fill_pred<8>(h, chroma_format_idc);
    else if (bit_depth == 9) fill_pred<9>(h, chroma_format_idc);
    else if (bit_depth == 10) fill_pred<10>(h, chroma_format_idc);
}

/* ------------------------------------------------------------------------- */
/* VideoDSPContext                                                             */
/* ------------------------------------------------------------------------- */
template <typename PX>
__global__ void __launch_bounds__(64)
k_emu_edge(PX *buf, int bpitch, const PX *region, int rpitch, int rx0, int ry0,
           int bw, int bh, int sx, int sy, int w, int h)
{
    /* region holds plane samples [rx0..] x [ry0..]; every output reads the plane at
     * clamped coordinates (videodsp_template.c:24-96) */
    for (int i = lane_id(); i < bw * bh; i += 64) {
        int y = i / bw, x = i - y * bw;
        int cx = clip3(sx + x, 0, w - 1), cy = clip3(sy + y, 0, h - 1);
        buf[y * bpitch + x] = region[(cy - ry0) * rpitch + (cx - rx0)];
    }
}
template <typename PX>
static void t1_emulated_edge_mc(uint8_t *buf, const uint8_t *src, ptrdiff_t buf_linesize, ptrdiff_t src_linesize,
                                int block_w, int block_h, int src_x, int src_y, int w, int h)
{
    constexpr int B = sizeof(PX);
    if (!w || !h) return;
    auto cl = [](int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); };
    /* the part of the plane the block can touch after clamping */
    const int rx0 = cl(src_x, 0, w - 1), rx1 = cl(src_x + block_w - 1, 0, w - 1);
    const int ry0 = cl(src_y, 0, h - 1), ry1 = cl(src_y + block_h - 1, 0, h - 1);
    const uint8_t *origin = src - src_y * src_linesize - (ptrdiff_t)src_x * B;
    for (int y0 = 0; y0 < block_h; y0 += 64) {        /* arena-sized strips; blocks are <= 71 rows */
        Arena &a = arena();
        const int bh = block_h - y0 < 64 ? block_h - y0 : 64;
        Win r = win_pack(a, origin + ry0 * src_linesize + rx0 * B, src_linesize, (rx1 - rx0 + 1) * B, ry1 - ry0 + 1);
        Win o = win_pack(a, nullptr, 0, block_w * B, bh, 0, 0);
        a.upload();
        LAUNCH1(k_emu_edge<PX>, a, a.d<PX>(o.off), o.pitch / B, a.d<PX>(r.off), r.pitch / B, rx0, ry0,
                block_w, bh, src_x, src_y + y0, w, h);
        a.download();
        win_unpack(a, o, buf + y0 * buf_linesize, buf_linesize, 0, 0, block_w * B, bh);
    }
}

void ff_videodsp_init_mi355x(VideoDSPContext *ctx, int bpc)
{
    /* the 8-bit form up to 8 bits per component, the 16-bit form above, as videodsp.c:40-44 selects them */
    if (bpc <= 8) ctx->emulated_edge_mc = t1_emulated_edge_mc<uint8_t>;
    else if (bpc <= 16) ctx->emulated_edge_mc = t1_emulated_edge_mc<uint16_t>;
    /* prefetch stays the C no-op: a host cache hint has no device meaning */
}
