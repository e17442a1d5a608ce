// bfgx_bispec.hpp -- bispectrum of a gridded 3-D map by the FFT estimator (Scoccimarro 2000; Sefusatti et al. 2016) for gfx950.
//
// For every k-bin i the half spectrum F of the map (bfgx_fft.hpp, kept whole this time) is filtered to the bin's shell and transformed
// back: I_i(x) = sum_{k in i} F(k) e^{+ikx} and, from a spectrum of ones, U_i(x) = sum_{k in i} e^{+ikx}.  Then
//     sum_x I_i I_j I_l / N^3 = sum of F(k1) F(k2) F(k3) over the closed triples k1 + k2 + k3 = 0 of the three bins,
//     sum_x U_i U_j U_l / N^3 = the number of such triples.
// The inverse transform reuses the forward kernels through IFFT(X) = conj(FFT(conj X)): the filter writes conj(F) [k in bin], the strided
// passes of bfgx_fft.hpp run as they are, and the last pass (complex to real along the contiguous axis, fft_c2r_lines_kernel) reads its
// input conjugated.  All transforms are unnormalised.
// The triple sums read every field value from HBM once, whatever the number of triangles (bispec_triangle_kernel), and are added
// in a fixed order (per-workgroup partials, bispec_finish_kernel): no floating-point atomics.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "bfgx_fft.hpp"

namespace bfgx {

constexpr int kBispecMaxBins = 32;
constexpr int kBispecMaxTri = 8192;
constexpr int kBispecThreads = 256;
constexpr int kBispecChunk = 128;          // points of all bins staged in LDS at a time (N^3 is a multiple of it: N >= 8)
static_assert(kBispecMaxBins * kBispecChunk % kBispecThreads == 0, "the staging loop moves whole rounds of the workgroup");
constexpr int kBispecMaxWgs = 512;         // workgroups of the triangle kernel at kBispecMaxPerThread sums per thread (what the partials in the work array are sized for; more with fewer sums)
// sums a thread of the triangle kernel holds at the most: (triangles + diagonal terms) / threads, rounded up
constexpr int kBispecMaxPerThread = (kBispecMaxTri + kBispecMaxBins + kBispecThreads - 1) / kBispecThreads;

// in-place complex conjugate of n values (the slab entries' inverse = conj, forward passes, conj)
__global__ void __launch_bounds__(256)
fft_conj_kernel(double2 *__restrict__ data, int64_t n)
{
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) data[i].y = -data[i].y;
}

// the k-shell filter: out = conj(spec) (unit: 1) where the mode (a, b, c) of the half spectrum [N][N][pitch] lies in bin `bin`, 0 elsewhere
// and in the pad columns.  The bin of a mode is looked up by n^2 = n_a^2 + n_b^2 + n_c^2 (integer wavevector) in the host-built byte table
// tab[3 (N/2)^2 + 1], 255 = outside the bins: the rule is evaluated once per n^2, on the host.
__global__ void __launch_bounds__(256)
bispec_select_kernel(const double2 *__restrict__ spec, double2 *__restrict__ out, const uint8_t *__restrict__ tab, int N, int pitch,
                     int bin, int unit)
{
    const int h = N >> 1;
    const unsigned total = (unsigned)N * N * pitch;                  // (at most 1024 * 1024 * 520 < 2^30)
    for (unsigned t = blockIdx.x * 256 + threadIdx.x; t < total; t += gridDim.x * 256) {
        const unsigned row = t / (unsigned)pitch;
        const int c = (int)(t - row * pitch);
        const int b = (int)(row & (N - 1)), a = (int)(row >> __builtin_ctz((unsigned)N));
        double2 v = make_double2(0.0, 0.0);
        if (c <= h) {
            const int na = a < h ? a : a - N, nb = b < h ? b : b - N;
            if (tab[na * na + nb * nb + c * c] == bin) {
                if (unit) v.x = 1.0;
                else { const double2 f = spec[t]; v = make_double2(f.x, -f.y); }
            }
        }
        out[t] = v;
    }
}

// the mirror of fft_r2c_lines_kernel: two adjacent rows A, B (the coefficients c <= N/2 of two real lines a, b) -> the lines, unnormalised.
// Z = A + i B is the spectrum of a + i b: Z_k = A_k + i B_k for k <= N/2 and Z_{N-k} = conj(A_k) + i conj(B_k); the forward transform of
// conj(Z) is conj(a + i b), so a = Re, b = -Im of one complex transform in LDS.  The rows hold the CONJUGATES of A and B (what the forward
// passes leave of a conjugated spectrum).  Columns c > N/2 (pad) are never read; the imaginary parts of c = 0 and c = N/2 are ignored,
// as numpy.irfft ignores them.
template <int PAIRS, int TPP>
__global__ void __launch_bounds__(PAIRS * TPP)
fft_c2r_lines_kernel(const double2 *__restrict__ in, double *__restrict__ map, int N, int log2n, const double2 *__restrict__ tw, int pitch)
{
    extern __shared__ double2 fbuf[];
    constexpr int H = TPP;
    const int sub = threadIdx.x / H, tid = threadIdx.x % H;
    const int64_t line = 2 * (PAIRS * (int64_t)blockIdx.x + sub);
    const double2 *sa = in + line * pitch, *sb = sa + pitch;
    double2 *fb = fbuf + (size_t)sub * N;
    const int h = N >> 1;
    for (int k = tid; k <= h; k += H) {
        double2 A = sa[k], B = sb[k];
        const bool edge = (k == 0 || k == h);
        A.y = edge ? 0.0 : -A.y;
        B.y = edge ? 0.0 : -B.y;
        fb[bit_reverse(k, log2n)] = make_double2(A.x - B.y, -(A.y + B.x));                  // conj(Z_k)
        if (!edge) fb[bit_reverse(N - k, log2n)] = make_double2(A.x + B.y, A.y - B.x);      // conj(Z_{N-k}) = A_k - i B_k
    }
    lds_fft_stages(fb, N, 1, tw, tid, H);
    double *da = map + line * N, *db = da + N;
    for (int i = tid; i < N; i += H) { const double2 w = fb[i]; da[i] = w.x; db[i] = -w.y; }
}

// LDS of the triangle kernel: a chunk of points x (nb bins + a column of ones)
__host__ __device__ inline size_t bispec_lds_bytes(int nb) { return sizeof(double) * (size_t)kBispecChunk * (nb + 1); }

// Triple sums over nb real fields [nb][npts].  A workgroup stages kBispecChunk points of ALL bins in LDS as [point / 2][bin][point % 2] (plus
// a column of ones at index nb) and every thread adds up the terms it owns from there: term e is the product of the columns (i, j, l) packed in
// ent[e] = i | j << 8 | l << 16 -- a triangle, or (i, i, nb) for the diagonal sum of I_i^2.  So a field value crosses HBM once per sweep
// however many triangles there are; the lanes of a wave read different columns of the SAME pair of points (distinct banks, equal
// addresses broadcast), and no sum is ever reduced across lanes.
//   TPT > 1: thread t owns the terms t, t + 256, ... (TPT of them, the missing ones read the ones column) over all points of the chunk;
//   TPT = 1: ntot <= 256 terms; G = the power of two >= ntot, 4 at the least; thread t owns term t % G over the pairs of points t / G, t / G + 256 / G, ...
// A thread keeps one running sum per term across the chunks its workgroup strides over (each chunk's sum is formed first and then added:
// the running sum takes one addition per chunk, not per point) and stores it to partials[workgroup][slot][thread] at the end.
template <int TPT>
__global__ void __launch_bounds__(kBispecThreads)
bispec_triangle_kernel(const double *__restrict__ fields, int64_t npts, int nb, const uint32_t *__restrict__ ent, int ntot, int G,
                       double *__restrict__ partials)
{
    extern __shared__ double sfl[];
    constexpr int NT = kBispecThreads;
    const int nbp = nb + 1, tid = threadIdx.x;
    const int p0 = TPT == 1 ? tid / G : 0, pstep = TPT == 1 ? NT / G : 1;
    uint32_t w[TPT];                                                 // the term's three columns, packed as in ent
    double acc[TPT];
#pragma unroll
    for (int k = 0; k < TPT; ++k) {
        const int e = TPT == 1 ? (tid & (G - 1)) : k * NT + tid;
        w[k] = e < ntot ? ent[e] : ((uint32_t)nb | (uint32_t)nb << 8 | (uint32_t)nb << 16);
        acc[k] = 0.0;
    }
    for (int p = tid; p < kBispecChunk; p += NT) sfl[((p >> 1) * nbp + nb) * 2 + (p & 1)] = 1.0;
    // staging: a thread moves the values t = tid, tid + 256, ... of the chunk's nb * kBispecChunk (bin t / kBispecChunk, point t % kBispecChunk).
    // They are fetched into registers, all loads in flight together, one chunk AHEAD: the next chunk's loads are issued before this chunk's
    // sums and land under them
    constexpr int NS = kBispecMaxBins * kBispecChunk / NT;
    const int nval = nb * kBispecChunk;
    double stage[NS];
    auto fetch = [&](int64_t ch) {
        const double *src = fields + ch * kBispecChunk;
#pragma unroll
        for (int u = 0; u < NS; ++u) {
            const int t = tid + u * NT;
            if (t < nval) stage[u] = src[(int64_t)(t / kBispecChunk) * npts + (t % kBispecChunk)];
        }
    };
    const int64_t nchunks = npts / kBispecChunk;
    if ((int64_t)blockIdx.x < nchunks) fetch(blockIdx.x);
    for (int64_t ch = blockIdx.x; ch < nchunks; ch += gridDim.x) {
        __syncthreads();                                             // (the previous chunk's readers are done)
#pragma unroll
        for (int u = 0; u < NS; ++u) {
            const int t = tid + u * NT;
            if (t < nval) sfl[(((t % kBispecChunk) >> 1) * nbp + t / kBispecChunk) * 2 + (t & 1)] = stage[u];
        }
        __syncthreads();
        if (ch + gridDim.x < nchunks) fetch(ch + gridDim.x);
        double loc[TPT];
#pragma unroll
        for (int k = 0; k < TPT; ++k) loc[k] = 0.0;
        for (int p = p0; p < kBispecChunk / 2; p += pstep) {             // (pairs of points: one 16-byte LDS read per column and pair)
            const double2 *row = reinterpret_cast<const double2 *>(sfl) + p * nbp;
#pragma unroll
            for (int k = 0; k < TPT; ++k) {
                const double2 a = row[w[k] & 255u], b = row[(w[k] >> 8) & 255u], c = row[w[k] >> 16];
                loc[k] += a.x * b.x * c.x;
                loc[k] += a.y * b.y * c.y;
            }
        }
#pragma unroll
        for (int k = 0; k < TPT; ++k) acc[k] += loc[k];
    }
#pragma unroll
    for (int k = 0; k < TPT; ++k) partials[((int64_t)blockIdx.x * TPT + k) * NT + tid] = acc[k];
}

// term e = blockIdx.x: the sum of its partials over the workgroups (and, TPT = 1, over the 256 / G point subsets) in a fixed order --
// thread t adds the rows t, t + 256, ... in ascending order, then a binary tree over the threads -- times `scale` (1 / N^3) into
// tri_out[e] (e < ntri) or diag_out[e - ntri]
__global__ void __launch_bounds__(256)
bispec_finish_kernel(const double *__restrict__ partials, int nwg, int tpt, int ntot, int G, int ntri, double scale,
                     double *__restrict__ tri_out, double *__restrict__ diag_out)
{
    __shared__ double ssum[256];
    const int e = blockIdx.x, t = threadIdx.x;
    const int nsub = tpt == 1 ? kBispecThreads / G : 1;
    const int nrows = nwg * nsub;
    double s = 0.0;
    for (int r = t; r < nrows; r += 256) {
        const int wg = r / nsub, sub = r - wg * nsub;
        const int64_t at = tpt == 1 ? (int64_t)wg * kBispecThreads + sub * G + e
                                    : ((int64_t)wg * tpt + e / kBispecThreads) * kBispecThreads + (e % kBispecThreads);
        s += partials[at];
    }
    ssum[t] = s;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (t < w) ssum[t] += ssum[t + w];
        __syncthreads();
    }
    if (t == 0) {
        const double v = ssum[0] * scale;
        if (e < ntri) tri_out[e] = v;
        else diag_out[e - ntri] = v;
    }
}

}  // namespace bfgx
