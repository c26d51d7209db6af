// Post-run kernels of a design loop on batched grids (include/fdtd2d_batch_design.h): the spectra of the recorded probe
// traces, a field's maximum per member, and the coefficient cells of a permittivity window.  None of them is a step
// kernel: the plain, monitored and point-source kernels keep their code.  Instantiated in batch_design.hip and reached
// through the launch functions at the end.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>

#include "kernels_batch_monitor.hpp"

namespace fdtd {

constexpr int BATCH_DSG_THREADS = 256;
constexpr int BATCH_SPEC_CHUNK = 32;      // samples staged in LDS per round

// max that keeps a NaN once it has seen one (on either side)
__device__ __forceinline__ double batch_nanmax(double m, double v) { return (v > m || v != v) ? v : m; }

// the workgroup's batch_nanmax; red: one double per wave.  The caller puts a barrier before red is used again.
__device__ __forceinline__ double batch_block_nanmax(double m, double *red)
{
    for (int off = 32; off > 0; off >>= 1) m = batch_nanmax(m, __shfl_xor(m, off));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
    __syncthreads();
    m = red[0];
    for (int w = 1; w < BATCH_DSG_THREADS / 64; ++w) m = batch_nanmax(m, red[w]);
    return m;
}

struct BatchSpectra {
    const double *trace;      // [member][probe][cap] (BatchMon::trace)
    const double *omega;      // count x nf, member-major
    double *re, *im;          // count x np x nf
    double *peak;             // count, or nullptr
    int B, np, nf;            // nf = 0: the peak alone
    long long cap, first, count;
    long long step0;          // sample n was recorded after step step0 + n + 1
    double dt;
};

// One workgroup per member.  The samples are walked in chunks of BATCH_SPEC_CHUNK: all threads evaluate the chunk's
// nf x chunk phasors once (batch_mon_phasor, the window DFT's expression) into LDS and stage its np x chunk trace
// samples with loads that are contiguous along n; then the thread of pair (p, k) adds the chunk to its two register
// accumulators in ascending n, the additions of BatchMon::add.  NQ pairs per thread (np * nf <= NQ * 256).
// LDS layout: samples [n][np | 1] (a wave's lanes read neighbouring probes of one n; the staging stores of one probe
// walk n with an odd stride in doubles, so 16 lanes hit 16 different bank pairs), phasors [n][k]{cos, -sin}.
template <int NQ>
__global__ __launch_bounds__(BATCH_DSG_THREADS) void k_batch_probe_spectra(BatchSpectra a)
{
    __shared__ double s_x[BATCH_SPEC_CHUNK * (BATCH_MON_MAX_PROBES + 1)];
    __shared__ double s_ph[BATCH_SPEC_CHUNK * BATCH_MON_MAX_FREQ * 2];
    __shared__ double s_red[BATCH_DSG_THREADS / 64];
    const int tid = threadIdx.x;
    const int ppad = a.np | 1, pf = a.np * a.nf;
    int qp[NQ], qk[NQ];       // the thread's pairs; a pair past the end works on (0, 0) and is not stored
#pragma unroll
    for (int j = 0; j < NQ; ++j) {
        const int q = tid + j * BATCH_DSG_THREADS;
        qp[j] = q < pf ? q / a.nf : 0;
        qk[j] = q < pf ? q % a.nf : 0;
    }
    for (int b = blockIdx.x; b < a.B; b += gridDim.x) {
        const double *tr = a.trace + (size_t)b * a.np * (size_t)a.cap + (size_t)a.first;
        double re[NQ], im[NQ];
#pragma unroll
        for (int j = 0; j < NQ; ++j) re[j] = im[j] = 0.0;
        double peak = 0.0;
        for (long long n0 = 0; n0 < a.count; n0 += BATCH_SPEC_CHUNK) {
            const int len = a.count - n0 < BATCH_SPEC_CHUNK ? (int)(a.count - n0) : BATCH_SPEC_CHUNK;
            for (int e = tid; e < len * a.nf; e += BATCH_DSG_THREADS) {
                const int n = e / a.nf, k = e - n * a.nf;
                batch_mon_phasor(s_ph + 2 * e, a.omega[(size_t)b * a.nf + k], a.step0 + a.first + n0 + n + 1, a.dt);
            }
            for (int e = tid; e < a.np * BATCH_SPEC_CHUNK; e += BATCH_DSG_THREADS) {
                const int p = e / BATCH_SPEC_CHUNK, n = e % BATCH_SPEC_CHUNK;
                if (n < len) {
                    const double x = tr[(size_t)p * (size_t)a.cap + (size_t)(n0 + n)];
                    s_x[n * ppad + p] = x;
                    peak = batch_nanmax(peak, fabs(x));
                }
            }
            __syncthreads();
            if (a.nf)
                for (int n = 0; n < len; ++n) {
#pragma unroll
                    for (int j = 0; j < NQ; ++j) {
                        const double x = s_x[n * ppad + qp[j]];
                        const double *ph = s_ph + 2 * (n * a.nf + qk[j]);
                        re[j] = re[j] + x * ph[0];
                        im[j] = im[j] + x * ph[1];
                    }
                }
            __syncthreads();
        }
#pragma unroll
        for (int j = 0; j < NQ; ++j) {
            const int q = tid + j * BATCH_DSG_THREADS;
            if (q < pf) {
                a.re[(size_t)b * pf + q] = re[j];
                a.im[(size_t)b * pf + q] = im[j];
            }
        }
        if (a.peak) {
            peak = batch_block_nanmax(peak, s_red);
            if (tid == 0) a.peak[b] = peak;
            __syncthreads();
        }
    }
}

// out[b] = max |f| over member b's nrows x ncols cells; one workgroup per member, a wave reduction at the end
template <class T>
__global__ __launch_bounds__(BATCH_DSG_THREADS) void k_batch_field_absmax(const T *__restrict__ f,
                                                                         double *__restrict__ out, int B, int nrows,
                                                                         int ncols, long long pitch, size_t mstride)
{
    __shared__ double s_red[BATCH_DSG_THREADS / 64];
    const int cells = nrows * ncols;
    for (int b = blockIdx.x; b < B; b += gridDim.x) {
        const T *m = f + (size_t)b * mstride;
        double v = 0.0;
        for (int t = threadIdx.x; t < cells; t += BATCH_DSG_THREADS) {
            const int i = t / ncols, j = t - i * ncols;
            v = batch_nanmax(v, fabs((double)m[(size_t)i * pitch + j]));
        }
        v = batch_block_nanmax(v, s_red);
        if (threadIdx.x == 0) out[b] = v;
        __syncthreads();
    }
}

// the coefficient cells of a window from its new eps (w: count x nr x nc in T): k_coef's expression, window cells only
template <class T>
__global__ __launch_bounds__(BATCH_DSG_THREADS) void k_batch_eps_window(T *__restrict__ ce, const T *__restrict__ w,
                                                                       int B, int r0, int c0, int nr, int nc,
                                                                       long long pitch, size_t mstride, T dt, T dx)
{
    const size_t W = (size_t)nr * nc, n = (size_t)B * W;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x; t < n; t += stride) {
        const size_t b = t / W;
        const int r = (int)(t - b * W), wi = r / nc, wj = r - wi * nc;
        const T x = w[t];
        ce[b * mstride + (size_t)(r0 + wi) * pitch + (c0 + wj)] = dt / (x * dx);
    }
}

// launches of the kernels above (batch_design.hip); dtype_f64: the engine's element type
void batch_probe_spectra_launch(const BatchSpectra &a, hipStream_t stream);
void batch_field_absmax_launch(const void *f, bool dtype_f64, double *out, int B, int nrows, int ncols, long long pitch,
                               size_t mstride, hipStream_t stream);
void batch_eps_window_launch(void *ce, const void *w, bool dtype_f64, int B, int r0, int c0, int nr, int nc,
                             long long pitch, size_t mstride, double dt, double dx, hipStream_t stream);

}  // namespace fdtd
