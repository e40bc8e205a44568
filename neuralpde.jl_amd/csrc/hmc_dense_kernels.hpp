// hmc_dense_kernels.hpp — the dense Euclidean metric of the resident HMC sampler (pinn_hmc_set_metric_dense).  The chain of
// hmc_kernels.hpp under a full inverse metric M^-1 = L L^T: r = L^-T z, theta += eps (M^-1 r), kinetic energy 1/2 r.(M^-1 r).  Selected on the host
// (hmc.cpp: Run); the energy and accept launches are those of hmc_kernels.hpp, k_hmc_energy taking v = M^-1 r.  M^-1 and L are [ld][ld] row-major,
// ld = P rounded up to 64, pads zero, L's strict upper zero.
//   k_hmc_dense_leap<T>    ONE launch per leapfrog step.  Every workgroup rebuilds the whole kicked momentum r' = r + kick g in LDS (g = hmc::logp_grad, as
//                          leap_body forms it), then forms its own 16 rows of v = M^-1 r': a wave takes 4 rows at a time, its lanes stride the columns (a row is
//                          read in whole 512-byte lines), lane partials, then the xor butterfly 32 ... 1.  Lanes 0..3 own the wave's rows: g_prop, r', v, and,
//                          drifting, theta and the evaluation's copy of it.  Momentum and theta PING-PONG between two buffers each (every workgroup reads
//                          all of r and theta): no workgroup reads in a launch what another writes in it.  DMODE_PRODUCT: v = M^-1 r alone.
//   k_hmc_dense_momentum   L^T r = z by back-substitution in ONE workgroup, 64-wide blocks from the last to the first: wave 0 solves the diagonal
//                          block in registers (lane j holds column j of the block and its right-hand side; 64 shuffle steps), then all four waves
//                          subtract the block's part from the right-hand side above it (thread t takes elements t, t + 256, ...; the block's 64
//                          unknowns in ascending order)
//   k_hmc_dense_chol_*     blocked right-looking Cholesky M^-1 = L L^T of the STAGED matrix, 64-column panels: _init copies the lower triangle; _panel
//                          (one workgroup) factorises the diagonal block in LDS and solves the rows below it, one row per thread; _trail (many
//                          workgroups, one wave per 16 x 16 tile on or below the diagonal) forms A22 -= L21 L21^T on v_mfma_f64_16x16x4_f64 (pk::mfma_f64).
//                          A pivot that is not positive and finite leaves flag = {1, its index}; every later launch returns at its first load.
//   k_hmc_dense_cov        the warm-up's window covariance: k_hmc_dense_mean (column means, rows in order, one thread per column), then one wave per
//                          lower 16 x 16 tile of C = (W - mu)^T (W - mu) on the f64 MFMA, K = the window's draws in order, the last K step zero-padded in
//                          registers; epilogue (k / (k + 5)) (C / k) + 1e-3 (5 / (k + 5)) I, mirrored into the upper tiles.  Reads the sample buffer in place.
//   k_hmc_dense_commit     flag clean: staged M^-1 and L replace the live pair, diag(M^-1) is kept for the callers' p-vector; else: the live pair stays
//                          and flag[DF_REJECTED] says so.  The host never has to know inside a warm-up.
// All sums have a fixed order and no atomics; contraction is off outside the MFMAs.  Every kernel has its PINN_EMU serial twin in the device's order.
#pragma once
#include "hmc_kernels.hpp"
#include "pinn_kernels5.hpp"

namespace hmc {

constexpr int DENSE_MAX_P = 4096;        // M^-1, L and their staged twins: 4 x 128 MiB there; a momentum vector: 32 KiB of LDS
constexpr int DB = 64;                   // block of the triangular solve and of the factorisation
constexpr int DT = 16;                   // MFMA tile
constexpr int LEAP_ROWS = 16;            // rows of v per workgroup: 4 waves x 4 rows
enum { DMODE_PRODUCT = 0, DMODE_FIRST = 1, DMODE_EVAL = 2 };
enum { DF_STATUS = 0, DF_INDEX = 1, DF_REJECTED = 2, DF_REJECTED_INDEX = 3, DF_COUNT = 4 };

struct Dense {
    int ld;                              // P rounded up to DB
    double* M; double* L;                // the live inverse metric and its lower factor
    double* Mn; double* Ln;              // staged: what pinn_hmc_set_metric_dense uploaded / the warm-up's covariance, and its factor
    double* v;                           // [P] M^-1 r
    double* mu;                          // [P] the window's column means
    double* diag;                        // [P] diag(M^-1)
    int* flag;                           // [DF_COUNT]
};
struct LeapIO {                          // the ping-pong pairs of one leap launch
    const double* th_in; double* th_out;
    const double* r_in; double* r_out;
};

inline int dense_ld(int P) { return (P + DB - 1) / DB * DB; }

// r'_i = r_i + kick g_i with leap_body's g; g and theta_i for the row's owner
template <class T> HMC_DEV double dense_kicked(int i, const Args& a, const T* ev, const LeapIO& io, int mode, double kick, double& g, double& x) {
    HMC_NO_CONTRACT
    g = 0.0; x = 0.0;
    if (mode == DMODE_PRODUCT) return io.r_in[i];
    if (mode == DMODE_FIRST) {
        g = a.g_cur[i];
        x = a.th_cur[i];
    } else {
        x = io.th_in[i];
        g = logp_grad<T>(i, a, ev, x);
    }
    return io.r_in[i] + kick * g;
}
// lane `lane`'s part of rows row0 .. row0 + 3 of M^-1 times the LDS copy of r'
HMC_DEV void dense_rows_partial(const Dense& dn, int row0, int lane, const double* sh, double (&acc)[4]) {
    HMC_NO_CONTRACT
    const double* m = dn.M + (size_t)row0 * (size_t)dn.ld;
    for (int k = 0; k < 4; ++k) acc[k] = 0.0;
    for (int j = lane; j < dn.ld; j += 64) {
        const double s = sh[j];
        for (int k = 0; k < 4; ++k) acc[k] += m[(size_t)k * (size_t)dn.ld + j] * s;
    }
}
template <class T> HMC_DEV void dense_owner(int i, const Args& a, const Dense& dn, const T* ev, const LeapIO& io, int mode, double kick, double eps, int drift, double vi) {
    HMC_NO_CONTRACT
    double g, x;
    const double r = dense_kicked<T>(i, a, ev, io, mode, kick, g, x);
    dn.v[i] = vi;
    if (mode == DMODE_PRODUCT) return;
    io.r_out[i] = r;
    if (mode == DMODE_EVAL) a.g_prop[i] = g;
    if (drift) {
        x = x + eps * vi;
        io.th_out[i] = x;
        if (a.th_eval64) a.th_eval64[i] = x;
        if (a.th_eval32) a.th_eval32[i] = (float)x;
    }
}
HMC_DEV void dense_mean_body(int i, int P, const Dense& dn, const double* samples, int w0, int w1) {
    HMC_NO_CONTRACT
    double s = 0.0;
    for (int row = w0; row < w1; ++row) s += samples[(size_t)row * P + i];
    dn.mu[i] = s / (double)(w1 - w0);
}
HMC_DEV void chol_init_body(size_t idx, const Dense& dn) {
    const size_t i = idx / (size_t)dn.ld, j = idx % (size_t)dn.ld;
    dn.Ln[idx] = j <= i ? dn.Mn[idx] : 0.0;
    if (idx == 0) { dn.flag[DF_STATUS] = 0; dn.flag[DF_INDEX] = -1; }      // (no launch reads the flag while this one runs)
}
HMC_DEV void commit_body(size_t idx, int P, const Dense& dn) {
    const size_t i = idx / (size_t)dn.ld, j = idx % (size_t)dn.ld;
    if (dn.flag[DF_STATUS] != 0) {
        if (idx == 0) { dn.flag[DF_REJECTED] = 1; dn.flag[DF_REJECTED_INDEX] = dn.flag[DF_INDEX]; }
        return;
    }
    const double m = dn.Mn[idx];
    dn.M[idx] = m;
    dn.L[idx] = dn.Ln[idx];
    if (i == j && (int)i < P) dn.diag[i] = m;
}

// ---- the two MFMA tiles: one wave each; device and emulation share the text (pk::LVd, PINN_LANES) ----
// A22[I.., J..] -= L21[I..] L21[J..]^T over the panel's 64 columns c0 ..; every index is below ld (pads are zero and stay zero)
HMC_DEV void chol_trail_tile(const Dense& dn, int c0, int I, int J) {
    const size_t ld = (size_t)dn.ld;
    pk::LVd<4> C;
    pk::LVd<1> A, B;
    PINN_LANES(l) {
        const int q = l >> 4, j = l & 15;
        for (int r = 0; r < 4; ++r) C(l, r) = dn.Ln[(size_t)(I + q + 4 * r) * ld + J + j];
    }
    for (int kb = 0; kb < DB / 4; ++kb) {
        PINN_LANES(l) {
            const int k = l >> 4, i = l & 15;
            A(l, 0) = -dn.Ln[(size_t)(I + i) * ld + c0 + 4 * kb + k];
            B(l, 0) = dn.Ln[(size_t)(J + i) * ld + c0 + 4 * kb + k];
        }
        pk::mfma_f64(C, 0, 1, A, 0, B, 0);
    }
    PINN_LANES(l) {
        const int q = l >> 4, j = l & 15;
        for (int r = 0; r < 4; ++r) dn.Ln[(size_t)(I + q + 4 * r) * ld + J + j] = C(l, r);
    }
}
// tile (I, J), J <= I, of the regularised window covariance into the staged matrix, and its mirror
HMC_DEV void cov_tile(int P, const Dense& dn, const double* samples, int w0, int w1, int I, int J) {
    HMC_NO_CONTRACT
    const size_t ld = (size_t)dn.ld;
    pk::LVd<4> C;
    pk::LVd<1> A, B;
    PINN_LANES(l) { for (int r = 0; r < 4; ++r) C(l, r) = 0.0; }
    for (int r0 = w0; r0 < w1; r0 += 4) {
        PINN_LANES(l) {
            const int row = r0 + (l >> 4), ca = I + (l & 15), cb = J + (l & 15);
            const bool ok = row < w1;                    // a window that is no multiple of 4 ends on zeros in registers
            A(l, 0) = ok && ca < P ? samples[(size_t)row * P + ca] - dn.mu[ca] : 0.0;
            B(l, 0) = ok && cb < P ? samples[(size_t)row * P + cb] - dn.mu[cb] : 0.0;
        }
        pk::mfma_f64(C, 0, 1, A, 0, B, 0);
    }
    const double k = (double)(w1 - w0);
    PINN_LANES(l) {
        const int q = l >> 4, j2 = J + (l & 15);
        for (int r = 0; r < 4; ++r) {
            const int i2 = I + q + 4 * r;
            if (i2 >= P || j2 >= P) continue;
            double val = (k / (k + 5.0)) * (C(l, r) / k);
            if (i2 == j2) val = val + 1e-3 * (5.0 / (k + 5.0));
            dn.Mn[(size_t)i2 * ld + j2] = val;
            if (I != J) dn.Mn[(size_t)j2 * ld + i2] = val;
        }
    }
}

#ifdef PINN_EMU
template <class T> inline void launch_dense_leap(const Args& a, const Dense& dn, const T* ev, const LeapIO& io, int mode, double kick, double eps, int from_sc, int drift, plat_stream) {
    HMC_NO_CONTRACT
    if (from_sc) { eps = a.sc[SC_EPS]; kick = kick * eps; }
    std::vector<double> sh((size_t)dn.ld, 0.0);
    for (int i = 0; i < a.P; ++i) { double g, x; sh[i] = dense_kicked<T>(i, a, ev, io, mode, kick, g, x); }
    std::vector<double> v((size_t)dn.ld, 0.0);
    for (int row0 = 0; row0 < a.P; row0 += 4) {
        double part[4][64];
        for (int l = 0; l < 64; ++l) {
            double acc[4];
            dense_rows_partial(dn, row0, l, sh.data(), acc);
            for (int k = 0; k < 4; ++k) part[k][l] = acc[k];
        }
        for (int k = 0; k < 4; ++k) v[row0 + k] = wave_butterfly(part[k]);
    }
    for (int i = 0; i < a.P; ++i) dense_owner<T>(i, a, dn, ev, io, mode, kick, eps, drift, v[i]);
}
inline void launch_dense_momentum(const Args& a, const Dense& dn, const double* z, uint64_t seed, unsigned draw, double* r_out, plat_stream) {
    HMC_NO_CONTRACT
    const unsigned key = rng_key((unsigned)seed, (unsigned)(seed >> 32), draw);
    const size_t ld = (size_t)dn.ld;
    std::vector<double> sh(ld, 0.0);
    for (int i = 0; i < a.P; ++i) sh[i] = z ? z[i] : rng_normal(key, (unsigned)i);
    for (int c0 = dn.ld - DB; c0 >= 0; c0 -= DB) {
        for (int ii = DB - 1; ii >= 0; --ii) {
            const double xi = c0 + ii < a.P ? sh[c0 + ii] / dn.L[(size_t)(c0 + ii) * ld + c0 + ii] : 0.0;
            sh[c0 + ii] = xi;
            for (int l = 0; l < ii; ++l) sh[c0 + l] = sh[c0 + l] - dn.L[(size_t)(c0 + ii) * ld + c0 + l] * xi;
        }
        for (int j = 0; j < c0; ++j) {
            double s = sh[j];
            for (int ii = 0; ii < DB; ++ii) s = s - dn.L[(size_t)(c0 + ii) * ld + j] * sh[c0 + ii];
            sh[j] = s;
        }
    }
    for (int i = 0; i < a.P; ++i) r_out[i] = sh[i];
}
inline void launch_chol(const Dense& dn, int P, plat_stream) {
    HMC_NO_CONTRACT
    const size_t ld = (size_t)dn.ld;
    for (size_t idx = ld * ld; idx-- > 0;) chol_init_body(idx, dn);
    for (int c0 = 0; c0 < dn.ld; c0 += DB) {
        if (dn.flag[DF_STATUS]) return;
        const int nv = std::min(DB, P - c0);
        double* blk = dn.Ln + (size_t)c0 * ld + c0;      // the diagonal block in place: the same element operations in the same order
        for (int c = 0; c < nv; ++c) {
            const double d = blk[(size_t)c * ld + c];
            if (!(d > 0.0) || !is_finite(d)) { dn.flag[DF_STATUS] = 1; dn.flag[DF_INDEX] = c0 + c; return; }
            const double s = sqrt(d);
            blk[(size_t)c * ld + c] = s;
            for (int i = c + 1; i < DB; ++i) blk[(size_t)i * ld + c] = blk[(size_t)i * ld + c] / s;
            for (int i = c + 1; i < DB; ++i)
                for (int j = c + 1; j <= i; ++j) blk[(size_t)i * ld + j] = blk[(size_t)i * ld + j] - blk[(size_t)i * ld + c] * blk[(size_t)j * ld + c];
        }
        for (int i = 0; i < DB; ++i)
            for (int j = i + 1; j < DB; ++j) blk[(size_t)i * ld + j] = 0.0;
        for (int i = c0 + DB; i < P; ++i) {
            double* row = dn.Ln + (size_t)i * ld + c0;
            for (int c = 0; c < DB; ++c) {
                double acc = row[c];
                for (int c2 = 0; c2 < c; ++c2) acc = acc - row[c2] * blk[(size_t)c * ld + c2];
                row[c] = acc / blk[(size_t)c * ld + c];
            }
        }
        const int off = c0 + DB;
        for (int I = off; I < dn.ld; I += DT)
            for (int J = off; J <= I; J += DT) chol_trail_tile(dn, c0, I, J);
    }
}
inline void launch_cov(const Args& a, const Dense& dn, const double* samples, int w0, int w1, plat_stream) {
    for (int i = 0; i < a.P; ++i) dense_mean_body(i, a.P, dn, samples, w0, w1);
    for (int I = 0; I < dn.ld; I += DT)
        for (int J = 0; J <= I; J += DT) cov_tile(a.P, dn, samples, w0, w1, I, J);
}
inline void launch_commit(const Args& a, const Dense& dn, plat_stream) {
    const size_t n = (size_t)dn.ld * (size_t)dn.ld;
    for (size_t idx = n; idx-- > 0;) commit_body(idx, a.P, dn);      // (element 0, which writes the rejection words, last)
}
#else
template <class T> __global__ void __launch_bounds__(BLOCK) k_hmc_dense_leap(const Args a, const Dense dn, const T* ev, const LeapIO io, int mode, double kick, double eps, int from_sc, int drift) {
    HMC_NO_CONTRACT
    extern __shared__ double dense_sh[];                 // [ld] the kicked momentum, pads zero
    if (from_sc) {
        eps = a.sc[SC_EPS];                              // (the same address in every lane)
        kick = kick * eps;
    }
    for (int i = (int)threadIdx.x; i < dn.ld; i += BLOCK) {
        double g, x;
        dense_sh[i] = i < a.P ? dense_kicked<T>(i, a, ev, io, mode, kick, g, x) : 0.0;
    }
    __syncthreads();
    const int lane = (int)threadIdx.x & 63, row0 = (int)blockIdx.x * LEAP_ROWS + ((int)threadIdx.x >> 6) * 4;      // (row0 + 3 < ld: ld is a multiple of 64)
    if (row0 >= a.P) return;
    double acc[4];
    dense_rows_partial(dn, row0, lane, dense_sh, acc);
    for (int m = 32; m >= 1; m >>= 1)
        for (int k = 0; k < 4; ++k) acc[k] += __shfl_xor(acc[k], m, 64);
    const double vi = lane == 0 ? acc[0] : lane == 1 ? acc[1] : lane == 2 ? acc[2] : acc[3];
    if (lane < 4 && row0 + lane < a.P) dense_owner<T>(row0 + lane, a, dn, ev, io, mode, kick, eps, drift, vi);
}
__global__ void __launch_bounds__(BLOCK) k_hmc_dense_momentum(const Args a, const Dense dn, const double* z, unsigned seed_lo, unsigned seed_hi, unsigned draw, double* r_out) {
    HMC_NO_CONTRACT
    extern __shared__ double dense_sh[];                 // [ld] the right-hand side, overwritten by the solution from the last block up
    const int tid = (int)threadIdx.x;
    const size_t ld = (size_t)dn.ld;
    const unsigned key = rng_key(seed_lo, seed_hi, draw);
    for (int i = tid; i < dn.ld; i += BLOCK) dense_sh[i] = i < a.P ? (z ? z[i] : rng_normal(key, (unsigned)i)) : 0.0;
    __syncthreads();
    for (int c0 = dn.ld - DB; c0 >= 0; c0 -= DB) {
        if (tid < 64) {                                  // wave 0: lane j holds L[c0 + ii][c0 + j], ii = 0..63 (zero above the diagonal), and element j
            double col[DB];
            PINN_UNROLL for (int ii = 0; ii < DB; ++ii) col[ii] = dn.L[(size_t)(c0 + ii) * ld + c0 + tid];
            double b = dense_sh[c0 + tid];
            PINN_UNROLL for (int ii = DB - 1; ii >= 0; --ii) {
                const double d = __shfl(col[ii], ii, 64), bi = __shfl(b, ii, 64);
                const double xi = c0 + ii < a.P ? bi / d : 0.0;
                if (tid == ii) b = xi;
                else if (tid < ii) b = b - col[ii] * xi;
            }
            dense_sh[c0 + tid] = b;
        }
        __syncthreads();
        for (int j = tid; j < c0; j += BLOCK) {
            double s = dense_sh[j];
            for (int ii = 0; ii < DB; ++ii) s = s - dn.L[(size_t)(c0 + ii) * ld + j] * dense_sh[c0 + ii];
            dense_sh[j] = s;
        }
        __syncthreads();
    }
    for (int i = tid; i < a.P; i += BLOCK) r_out[i] = dense_sh[i];
}
__global__ void __launch_bounds__(BLOCK) k_hmc_dense_chol_init(const Dense dn) {
    const size_t idx = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    if (idx < (size_t)dn.ld * (size_t)dn.ld) chol_init_body(idx, dn);
}
__global__ void __launch_bounds__(BLOCK) k_hmc_dense_chol_panel(const Dense dn, int P, int c0) {
    HMC_NO_CONTRACT
    __shared__ double blk[DB][DB + 1];
    if (dn.flag[DF_STATUS] != 0) return;                 // written by an earlier launch
    const int tid = (int)threadIdx.x, nv = min(DB, P - c0);
    const size_t ld = (size_t)dn.ld;
    for (int idx = tid; idx < DB * DB; idx += BLOCK) blk[idx >> 6][idx & 63] = dn.Ln[(size_t)(c0 + (idx >> 6)) * ld + c0 + (idx & 63)];
    __syncthreads();
    for (int c = 0; c < nv; ++c) {
        const double d = blk[c][c];
        if (!(d > 0.0) || !is_finite(d)) {               // (the same d in every thread: the whole workgroup leaves)
            if (tid == 0) { dn.flag[DF_STATUS] = 1; dn.flag[DF_INDEX] = c0 + c; }
            return;
        }
        __syncthreads();
        const double s = sqrt(d);
        if (tid == c) blk[c][c] = s;
        else if (tid > c && tid < DB) blk[tid][c] = blk[tid][c] / s;
        __syncthreads();
        for (int idx = tid; idx < DB * DB; idx += BLOCK) {
            const int i = idx >> 6, j = idx & 63;
            if (j > c && i >= j) blk[i][j] = blk[i][j] - blk[i][c] * blk[j][c];
        }
        __syncthreads();
    }
    for (int idx = tid; idx < DB * DB; idx += BLOCK) {
        const int i = idx >> 6, j = idx & 63;
        dn.Ln[(size_t)(c0 + i) * ld + c0 + j] = j <= i ? blk[i][j] : 0.0;
    }
    for (int i = c0 + DB + tid; i < P; i += BLOCK) {     // the rows below: x L_kk^T = a, one row per thread, the row in registers
        double* row = dn.Ln + (size_t)i * ld + c0;
        double x[DB];
        PINN_UNROLL for (int c = 0; c < DB; ++c) x[c] = row[c];
        PINN_UNROLL for (int c = 0; c < DB; ++c) {
            double acc = x[c];
            PINN_UNROLL for (int c2 = 0; c2 < c; ++c2) acc = acc - x[c2] * blk[c][c2];
            x[c] = acc / blk[c][c];
        }
        PINN_UNROLL for (int c = 0; c < DB; ++c) row[c] = x[c];
    }
}
__global__ void __launch_bounds__(BLOCK) k_hmc_dense_chol_trail(const Dense dn, int c0) {
    if (dn.flag[DF_STATUS] != 0) return;                 // written by an earlier launch
    const int off = c0 + DB, ti = (int)blockIdx.x, tj = (int)blockIdx.y * (BLOCK / 64) + ((int)threadIdx.x >> 6);
    if (tj > ti) return;
    chol_trail_tile(dn, c0, off + DT * ti, off + DT * tj);
}
__global__ void __launch_bounds__(BLOCK) k_hmc_dense_mean(const Args a, const Dense dn, const double* samples, int w0, int w1) {
    const int i = (int)(blockIdx.x * BLOCK + threadIdx.x);
    if (i < a.P) dense_mean_body(i, a.P, dn, samples, w0, w1);
}
__global__ void __launch_bounds__(BLOCK) k_hmc_dense_cov(const Args a, const Dense dn, const double* samples, int w0, int w1) {
    const int ti = (int)blockIdx.x, tj = (int)blockIdx.y * (BLOCK / 64) + ((int)threadIdx.x >> 6);
    if (tj > ti) return;
    cov_tile(a.P, dn, samples, w0, w1, DT * ti, DT * tj);
}
__global__ void __launch_bounds__(BLOCK) k_hmc_dense_commit(const Args a, const Dense dn) {
    const size_t idx = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    if (idx < (size_t)dn.ld * (size_t)dn.ld) commit_body(idx, a.P, dn);
}
template <class T> inline void launch_dense_leap(const Args& a, const Dense& dn, const T* ev, const LeapIO& io, int mode, double kick, double eps, int from_sc, int drift, plat_stream st) {
    hipLaunchKernelGGL(k_hmc_dense_leap<T>, dim3((a.P + LEAP_ROWS - 1) / LEAP_ROWS), dim3(BLOCK), sizeof(double) * (size_t)dn.ld, st, a, dn, ev, io, mode, kick, eps, from_sc, drift);
}
inline void launch_dense_momentum(const Args& a, const Dense& dn, const double* z, uint64_t seed, unsigned draw, double* r_out, plat_stream st) {
    hipLaunchKernelGGL(k_hmc_dense_momentum, dim3(1), dim3(BLOCK), sizeof(double) * (size_t)dn.ld, st, a, dn, z, (unsigned)seed, (unsigned)(seed >> 32), draw, r_out);
}
inline unsigned dense_elem_blocks(const Dense& dn) { return (unsigned)(((size_t)dn.ld * (size_t)dn.ld + BLOCK - 1) / BLOCK); }
inline void launch_chol(const Dense& dn, int P, plat_stream st) {
    hipLaunchKernelGGL(k_hmc_dense_chol_init, dim3(dense_elem_blocks(dn)), dim3(BLOCK), 0, st, dn);
    for (int c0 = 0; c0 < dn.ld; c0 += DB) {
        hipLaunchKernelGGL(k_hmc_dense_chol_panel, dim3(1), dim3(BLOCK), 0, st, dn, P, c0);
        const int nt = (dn.ld - c0 - DB) / DT;
        if (nt > 0) hipLaunchKernelGGL(k_hmc_dense_chol_trail, dim3(nt, (nt + 3) / 4), dim3(BLOCK), 0, st, dn, c0);
    }
}
inline void launch_cov(const Args& a, const Dense& dn, const double* samples, int w0, int w1, plat_stream st) {
    hipLaunchKernelGGL(k_hmc_dense_mean, dim3((a.P + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, st, a, dn, samples, w0, w1);
    const int nt = dn.ld / DT;
    hipLaunchKernelGGL(k_hmc_dense_cov, dim3(nt, (nt + 3) / 4), dim3(BLOCK), 0, st, a, dn, samples, w0, w1);
}
inline void launch_commit(const Args& a, const Dense& dn, plat_stream st) {
    hipLaunchKernelGGL(k_hmc_dense_commit, dim3(dense_elem_blocks(dn)), dim3(BLOCK), 0, st, a, dn);
}
#endif

}  // namespace hmc
