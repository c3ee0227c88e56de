// pcl_kernel_variational.hpp -- the variational (sensitivity) integrators of batch_mode PCL_BATCH_VARIATIONAL (gfx950; included by
// piccolo_hip.hip, and compiled on its own by tests/test_variational_cpu.py for its resource check).
//
// The state of one knot is [X; Xv_1; ...; Xv_v] (the reference's vcat of the state and its variations, src/control/integrators.jl:234-264), acted on
// per state column by the lifted generator  Ghat = var_G(G, [Gv_i])  = [[G, 0, ...], [Gv_1, G, 0, ...], ..., [Gv_v, 0, ..., G]]
// (isomorphisms.jl:398-422).  With T_j = c_j h^j and Y_j = (-1)^j X'_{k+1} - X'_k (lifted), the residual is  delta' = sum_j T_j Ghat^j Y_j.
//
// Two roles per interval in one launch (pcl_var_fused_kernel):
//   * block workgroups fold the powers P_j = G^j and the Frechet powers Q_j^i (the (i,0) block of Ghat^j: Q_1 = Gv_i, Q_j = G Q_{j-1} + Gv_i P_{j-1})
//     into B^{+-} = sum_j T_j (+-1)^j P_j and L^{+-}_i = sum_{j>=1} T_j (+-1)^j Q_j^i, and stream their d replicated copies with 16-byte stores
//     (a compact launch, VarParams::compact: each of the 2 + 2 v tiles once, from the same registers, and the tails right behind them);
//   * column workgroups run one wave per state column: lane i holds row i of each of the 1 + v components, products with G / Gv_i / G_l are
//     lane-parallel row-compressed (ELL) products: lane i sums its row's non-zeros, the entries of x fetched from their lanes.  They write delta and the tails
//     (d delta / d u_l, d delta / d dt), from the Horner chains  R_{q-1} = T_q Y_q,  R_e = Ghat R_{e+1} + T_{e+1} Y_{e+1}:
//         delta' = Y_0 + Ghat R_0,   d delta' / d u_l = sum_e Ghat^e Ghat_l R_e,   d delta' / d h = sum_j T'_j Ghat^j Y_j   (Ghat_l = I (x) G_l).
// No two workgroups share an output and none waits for another: the values do not depend on how the columns and the copies are split.
//
// pcl_var_hess_kernel: one workgroup per interval, one wave per state column at a time, the transposed chains on the lifted multipliers M:
//     W_0 = M, W_j = Ghat^T W_{j-1};  V_{l,1} = Ghat_l^T M, V_{l,j} = Ghat^T V_{l,j-1} + Ghat_l^T W_{j-1}       (Ghat^T y = [G^T y_0 + sum_i Gv_i^T y_i; G^T y_i])
//     (u_i,u_l) = sum_{e=1}^{q-1} <V_{i,e}, Ghat_l R_e> + <V_{l,e}, Ghat_i R_e>    (h,u_l) = sum_j T'_j <V_{l,j}, Y_j>    (h,h) = sum_j T''_j <W_j, Y_j>
//     d2/du_l dX_k = -sum_j T_j V_{l,j}, d2/du_l dX_{k+1} = sum_j T_j (-1)^j V_{l,j}; d2/dh dX the same with T'_j and W_j.
// The V_{l,j} of a column stay in LDS (one slab per wave); the scalar entries are summed per wave in a fixed order, then over the waves.
#pragma once

#define PCL_VAR_MAXV 2      // variations per context (v = 1, 2)
#define PCL_VAR_THREADS 512 // threads of a fused-kernel workgroup (8 waves)
#define PCL_VAR_PPT 4       // B / L value pairs per thread of a block workgroup: (n*n/2) / 512 <= 4 for n <= 64

typedef double pcl_var_d2 __attribute__((ext_vector_type(2)));

struct VarParams {
    const double *Z;
    const double *mu;
    double *delta;      // may be null
    double *vals;       // may be null (residual only)
    double *hess;
    const double *G0;   // n*n column-major: the drift
    const double *Gj;   // [m][n*n]: the drives
    const double *Gv;   // [v][n*n]: the scaled variation generators
    const double *G0T;  // transposes of the same
    const double *GjT;
    const double *GvT;
    long long jper, hper;  // values per interval
    int n, cols, m, K, z_dim, u_off, dt_off;
    int xo[PCL_VAR_MAXV + 1];  // state offsets of the 1 + v components inside a knot
    int nbw, ncw;  // block / column workgroups per interval (fused kernel)
    int hw;        // waves per workgroup (Hessian kernel)
    int compact;   // fused kernel (option var_compact): the values are [-B+ | B- | per variation: -L+_i | L-_i | tails], every tile once (nbw = 1)
    // column role: the generators row-compressed (ELL, [slot t][row i], padded with column 0 / value 0), so a product costs its
    // non-zeros per row instead of n: G(u) on the union pattern of the drift and the drives (gval: the drift's values, then each drive's),
    // the drives, the variation generators
    const int *gcol, *dcol, *vcol;
    const double *gval, *dval, *vval;
    int wG, wD, wV;
    double c[6];   // diagonal Pade coefficients c_0 .. c_q
};

// x[k] of the wave (k uniform)
__device__ __forceinline__ double pcl_var_bcast(double x, int k) {
    const int lo = __builtin_amdgcn_readlane(__double2loint(x), k);
    const int hi = __builtin_amdgcn_readlane(__double2hiint(x), k);
    return __hiloint2double(hi, lo);
}

// out[b] = A x[b] for b < NB (A: n x n column-major, lane i = row i; lanes >= n hold 0)
template <int NB>
__device__ __forceinline__ void pcl_var_mv(const double *__restrict__ A, int n, int lane, const double *x, double *out) {
    double acc[NB];
#pragma unroll
    for (int b = 0; b < NB; ++b) acc[b] = 0.0;
    const bool on = lane < n;
    const double *a = A + (on ? lane : 0);
    for (int k = 0; k < n; ++k) {
        const double ak = on ? a[(size_t)k * n] : 0.0;
#pragma unroll
        for (int b = 0; b < NB; ++b) acc[b] = fma(ak, pcl_var_bcast(x[b], k), acc[b]);
    }
#pragma unroll
    for (int b = 0; b < NB; ++b) out[b] = acc[b];
}

// lifted forward product  out = Ghat x  (G in LDS, Gv in LDS or global)
template <int V>
__device__ __forceinline__ void pcl_var_fwd(const double *G, const double *Gv, int n, int lane, const double *x, double *out) {
    pcl_var_mv<V + 1>(G, n, lane, x, out);
#pragma unroll
    for (int i = 1; i <= V; ++i) {
        double t;
        pcl_var_mv<1>(Gv + (size_t)(i - 1) * n * n, n, lane, x, &t);
        out[i] += t;
    }
}
// lifted adjoint product  out = Ghat^T y  (GT = G^T, GvT = Gv_i^T)
template <int V>
__device__ __forceinline__ void pcl_var_adj(const double *GT, const double *GvT, int n, int lane, const double *y, double *out) {
    pcl_var_mv<V + 1>(GT, n, lane, y, out);
#pragma unroll
    for (int i = 1; i <= V; ++i) {
        double t;
        pcl_var_mv<1>(GvT + (size_t)(i - 1) * n * n, n, lane, y + i, &t);
        out[0] += t;
    }
}

struct VarEll {
    const double *val;  // [w][n]
    const int *col;     // [w][n]
    int w;
};
// out[b] = A x[b] for a row-compressed A: lane i sums val[t][i] x[col[t][i]] (the entries of x fetched from their lanes)
template <int NB>
__device__ __forceinline__ void pcl_var_spmv(const VarEll &A, int n, int lane, const double *x, double *out) {
    double acc[NB];
#pragma unroll
    for (int b = 0; b < NB; ++b) acc[b] = 0.0;
    const bool on = lane < n;
    const int li = on ? lane : 0;
    for (int t = 0; t < A.w; ++t) {
        const double a = on ? A.val[(size_t)t * n + li] : 0.0;
        const int c = A.col[(size_t)t * n + li];
#pragma unroll
        for (int b = 0; b < NB; ++b) acc[b] = fma(a, __shfl(x[b], c, 64), acc[b]);
    }
#pragma unroll
    for (int b = 0; b < NB; ++b) out[b] = acc[b];
}
// lifted forward product out = Ghat x with the row-compressed G(u) and Gv_i
template <int V>
__device__ __forceinline__ void pcl_var_fwd_ell(const VarEll &G, const VarParams &p, int n, int lane, const double *x, double *out) {
    pcl_var_spmv<V + 1>(G, n, lane, x, out);
#pragma unroll
    for (int i = 1; i <= V; ++i) {
        const VarEll Gv = {p.vval + (size_t)(i - 1) * p.wV * n, p.vcol + (size_t)(i - 1) * p.wV * n, p.wV};
        double t;
        pcl_var_spmv<1>(Gv, n, lane, x, &t);
        out[i] += t;
    }
}

// T_j = c_j h^j, T'_j = j c_j h^(j-1), T''_j = j (j-1) c_j h^(j-2) (products, no division: h = 0 is allowed)
template <int Q>
__device__ __forceinline__ void pcl_var_coeffs(const double *c, double h, double *T, double *T1, double *T2) {
#pragma unroll
    for (int j = 0; j <= Q; ++j) {
        double a = c[j], b = j * c[j], e = j * (j - 1) * c[j];
#pragma unroll
        for (int r = 0; r < j; ++r) a *= h;
#pragma unroll
        for (int r = 0; r + 1 < j; ++r) b *= h;
#pragma unroll
        for (int r = 0; r + 2 < j; ++r) e *= h;
        T[j] = a;
        T1[j] = b;
        T2[j] = e;
    }
}

__device__ __forceinline__ double pcl_var_wave_sum(double x) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o, 64);
    return x;
}

// ---------------------------------------------------------------------------------------------------------------------------------------------
// Fused residual + Jacobian (JAC = false: residual only -- the column workgroups without the tails, no block workgroups)
// grid = K * (nbw + ncw) (JAC) or K * ncw; block = PCL_VAR_THREADS; LDS: (2 + V) n*n doubles (block role) / wG n (column role)
// ---------------------------------------------------------------------------------------------------------------------------------------------
template <int V, int Q>
__device__ void pcl_var_block_role(const VarParams &p, int k, int rb, double *lds) {
    const int n = p.n, nn = n * n, npair = nn >> 1, C = p.cols;
    const int tid = threadIdx.x;
    double *G = lds, *P = lds + nn, *Qm = lds + 2 * nn;  // Qm: V tiles
    const double *z = p.Z + (size_t)k * p.z_dim;
    const double h = z[p.dt_off];
    double T[Q + 1], T1[Q + 1], T2[Q + 1];
    pcl_var_coeffs<Q>(p.c, h, T, T1, T2);
    // G = G0 + sum_l u_l G_l; P_1 = G; Q_1^i = Gv_i (this thread's pairs)
    pcl_var_d2 pc[PCL_VAR_PPT], qc[PCL_VAR_PPT][V > 0 ? V : 1];
    pcl_var_d2 E[PCL_VAR_PPT], O[PCL_VAR_PPT], EQ[PCL_VAR_PPT][V], OQ[PCL_VAR_PPT][V];
#pragma unroll
    for (int s = 0; s < PCL_VAR_PPT; ++s) {
        const int pr = tid + s * PCL_VAR_THREADS;
        if (pr < npair) {
            const int e = 2 * pr;
            pcl_var_d2 a = *(const pcl_var_d2 *)(p.G0 + e);
            for (int l = 0; l < p.m; ++l) a += z[p.u_off + l] * *(const pcl_var_d2 *)(p.Gj + (size_t)l * nn + e);
            pc[s] = a;
            *(pcl_var_d2 *)(G + e) = a;
            *(pcl_var_d2 *)(P + e) = a;
            const int i = e % n, j = e / n;
            pcl_var_d2 eye = {i == j ? 1.0 : 0.0, i + 1 == j ? 1.0 : 0.0};
            E[s] = eye;  // T_0 P_0 = I
            O[s] = T[1] * a;
#pragma unroll
            for (int v = 0; v < V; ++v) {
                const pcl_var_d2 b = *(const pcl_var_d2 *)(p.Gv + (size_t)v * nn + e);
                qc[s][v] = b;
                *(pcl_var_d2 *)(Qm + (size_t)v * nn + e) = b;
                EQ[s][v] = pcl_var_d2{0.0, 0.0};
                OQ[s][v] = T[1] * b;
            }
        }
    }
    __syncthreads();
#pragma unroll
    for (int j = 2; j <= Q; ++j) {
        // P_j = G P_{j-1},  Q_j^i = G Q_{j-1}^i + Gv_i P_{j-1}
#pragma unroll
        for (int s = 0; s < PCL_VAR_PPT; ++s) {
            const int pr = tid + s * PCL_VAR_THREADS;
            if (pr < npair) {
                const int e = 2 * pr, i = e % n, c = e / n;
                pcl_var_d2 ap = {0.0, 0.0}, aq[V];
#pragma unroll
                for (int v = 0; v < V; ++v) aq[v] = pcl_var_d2{0.0, 0.0};
                for (int kk = 0; kk < n; ++kk) {
                    const pcl_var_d2 gi = *(const pcl_var_d2 *)(G + (size_t)kk * n + i);
                    const double pk = P[(size_t)c * n + kk];
                    ap += gi * pk;
#pragma unroll
                    for (int v = 0; v < V; ++v) {
                        const pcl_var_d2 gv = *(const pcl_var_d2 *)(p.Gv + (size_t)v * nn + (size_t)kk * n + i);
                        aq[v] += gi * Qm[(size_t)v * nn + (size_t)c * n + kk] + gv * pk;
                    }
                }
                pc[s] = ap;
#pragma unroll
                for (int v = 0; v < V; ++v) qc[s][v] = aq[v];
                if (j & 1) {
                    O[s] += T[j] * ap;
#pragma unroll
                    for (int v = 0; v < V; ++v) OQ[s][v] += T[j] * aq[v];
                } else {
                    E[s] += T[j] * ap;
#pragma unroll
                    for (int v = 0; v < V; ++v) EQ[s][v] += T[j] * aq[v];
                }
            }
        }
        if (j < Q) {
            __syncthreads();
#pragma unroll
            for (int s = 0; s < PCL_VAR_PPT; ++s) {
                const int pr = tid + s * PCL_VAR_THREADS;
                if (pr < npair) {
                    *(pcl_var_d2 *)(P + 2 * pr) = pc[s];
#pragma unroll
                    for (int v = 0; v < V; ++v) *(pcl_var_d2 *)(Qm + (size_t)v * nn + 2 * pr) = qc[s][v];
                }
            }
            __syncthreads();
        }
    }
    double *base = p.vals + (size_t)k * p.jper;
    if (p.compact) {  // [-B+ | B- | -L+_1 | L-_1 | ..]: every tile once (one block workgroup per interval)
#pragma unroll
        for (int s = 0; s < PCL_VAR_PPT; ++s) {
            const int pr = tid + s * PCL_VAR_THREADS;
            if (pr < npair) {
                double *b0 = base + 2 * pr;
                const pcl_var_d2 bp = E[s] + O[s], bm = E[s] - O[s];
                *(pcl_var_d2 *)b0 = -bp;
                *(pcl_var_d2 *)(b0 + nn) = bm;
#pragma unroll
                for (int v = 0; v < V; ++v) {
                    *(pcl_var_d2 *)(b0 + (size_t)(2 + 2 * v) * nn) = -(EQ[s][v] + OQ[s][v]);
                    *(pcl_var_d2 *)(b0 + (size_t)(3 + 2 * v) * nn) = EQ[s][v] - OQ[s][v];
                }
            }
        }
        return;
    }
    // the copies c in [c0, c1) of every block of this interval
    const int c0 = (int)((long long)rb * C / p.nbw), c1 = (int)((long long)(rb + 1) * C / p.nbw);
    const long long segsz = (long long)C * nn;
    for (int c = c0; c < c1; ++c) {
        double *b0 = base + (size_t)c * nn;
#pragma unroll
        for (int s = 0; s < PCL_VAR_PPT; ++s) {
            const int pr = tid + s * PCL_VAR_THREADS;
            if (pr < npair) {
                const int e = 2 * pr;
                const pcl_var_d2 bp = E[s] + O[s], bm = E[s] - O[s];
                __builtin_nontemporal_store(-bp, (pcl_var_d2 *)(b0 + e));
                __builtin_nontemporal_store(bm, (pcl_var_d2 *)(b0 + segsz + e));
#pragma unroll
                for (int v = 0; v < V; ++v) {
                    double *bv = b0 + (2 + 4 * v) * segsz + e;
                    __builtin_nontemporal_store(-bp, (pcl_var_d2 *)bv);
                    __builtin_nontemporal_store(bm, (pcl_var_d2 *)(bv + segsz));
                    __builtin_nontemporal_store(-(EQ[s][v] + OQ[s][v]), (pcl_var_d2 *)(bv + 2 * segsz));
                    __builtin_nontemporal_store(EQ[s][v] - OQ[s][v], (pcl_var_d2 *)(bv + 3 * segsz));
                }
            }
        }
    }
}

template <int V, int Q, bool JAC>
__device__ void pcl_var_col_role(const VarParams &p, int k, int rc, double *lds) {
    const int n = p.n, nn = n * n, C = p.cols, m = p.m;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = PCL_VAR_THREADS / 64;
    const double *z0 = p.Z + (size_t)k * p.z_dim, *z1 = z0 + p.z_dim;
    // G(u_k) on the union pattern of the drift and the drives: gvals[t][i] = G0 + sum_l u_l G_l at (i, gcol[t][i])
    double *gv = lds;
    const int ng = p.wG * n;
    for (int e = threadIdx.x; e < ng; e += PCL_VAR_THREADS) {
        double a = p.gval[e];
        for (int l = 0; l < m; ++l) a = fma(z0[p.u_off + l], p.gval[(size_t)(l + 1) * ng + e], a);
        gv[e] = a;
    }
    __syncthreads();
    const VarEll G = {gv, p.gcol, p.wG};
    const double h = z0[p.dt_off];
    double T[Q + 1], T1[Q + 1], T2[Q + 1];
    pcl_var_coeffs<Q>(p.c, h, T, T1, T2);
    const int ca = (int)((long long)rc * C / p.ncw), cb = (int)((long long)(rc + 1) * C / p.ncw);
    const long long xdc = (long long)n * C, xdl = xdc * (V + 1);
    const bool on = lane < n;
    for (int c = ca + wave; c < cb; c += nw) {
        double Ye[V + 1], Yo[V + 1];
#pragma unroll
        for (int b = 0; b <= V; ++b) {
            const double x0 = on ? z0[p.xo[b] + (size_t)c * n + lane] : 0.0;
            const double x1 = on ? z1[p.xo[b] + (size_t)c * n + lane] : 0.0;
            Ye[b] = x1 - x0;
            Yo[b] = -x1 - x0;
        }
        double R[Q][V + 1], t[V + 1];
#pragma unroll
        for (int b = 0; b <= V; ++b) R[Q - 1][b] = T[Q] * ((Q & 1) ? Yo[b] : Ye[b]);
#pragma unroll
        for (int e = Q - 2; e >= 0; --e) {
            pcl_var_fwd_ell<V>(G, p, n, lane, R[e + 1], t);
#pragma unroll
            for (int b = 0; b <= V; ++b) R[e][b] = fma(T[e + 1], ((e + 1) & 1) ? Yo[b] : Ye[b], t[b]);
        }
        pcl_var_fwd_ell<V>(G, p, n, lane, R[0], t);
        if (p.delta && on) {
#pragma unroll
            for (int b = 0; b <= V; ++b) p.delta[(size_t)k * xdl + b * xdc + (size_t)c * n + lane] = t[b] + Ye[b];
        }
        if (!JAC) continue;
        double *tail = p.vals + (size_t)k * p.jper + (p.compact ? (size_t)(2 + 2 * V) * nn : (size_t)(2 + 4 * V) * C * nn);
        const long long tstride = (long long)(m + 1) * n;  // per (component, column)
        // d/dh: Horner on T'_j
        double R1[V + 1];
#pragma unroll
        for (int b = 0; b <= V; ++b) R1[b] = T1[Q] * ((Q & 1) ? Yo[b] : Ye[b]);
#pragma unroll
        for (int e = Q - 2; e >= 0; --e) {
            pcl_var_fwd_ell<V>(G, p, n, lane, R1, t);
#pragma unroll
            for (int b = 0; b <= V; ++b) R1[b] = fma(T1[e + 1], ((e + 1) & 1) ? Yo[b] : Ye[b], t[b]);
        }
        pcl_var_fwd_ell<V>(G, p, n, lane, R1, t);
        if (on) {
#pragma unroll
            for (int b = 0; b <= V; ++b) __builtin_nontemporal_store(t[b], tail + ((size_t)b * C + c) * tstride + (size_t)m * n + lane);
        }
        for (int l = 0; l < m; ++l) {
            const VarEll Gl = {p.dval + (size_t)l * p.wD * n, p.dcol + (size_t)l * p.wD * n, p.wD};
            double acc[V + 1], s[V + 1];
            pcl_var_spmv<V + 1>(Gl, n, lane, R[Q - 1], acc);
#pragma unroll
            for (int e = Q - 2; e >= 0; --e) {
                pcl_var_fwd_ell<V>(G, p, n, lane, acc, t);
                pcl_var_spmv<V + 1>(Gl, n, lane, R[e], s);
#pragma unroll
                for (int b = 0; b <= V; ++b) acc[b] = t[b] + s[b];
            }
            if (on) {
#pragma unroll
                for (int b = 0; b <= V; ++b) __builtin_nontemporal_store(acc[b], tail + ((size_t)b * C + c) * tstride + (size_t)l * n + lane);
            }
        }
    }
}

template <int V, int Q, bool JAC>
__global__ void __launch_bounds__(PCL_VAR_THREADS) pcl_var_fused_kernel(VarParams p) {
    extern __shared__ double pcl_var_lds[];
    const int per = JAC ? p.nbw + p.ncw : p.ncw;
    const int k = blockIdx.x / per, r = blockIdx.x % per;
    if (k >= p.K) return;
    if (JAC && r < p.nbw)
        pcl_var_block_role<V, Q>(p, k, r, pcl_var_lds);
    else
        pcl_var_col_role<V, Q, JAC>(p, k, JAC ? r - p.nbw : r, pcl_var_lds);
}

// ---------------------------------------------------------------------------------------------------------------------------------------------
// Hessian of the Lagrangian: grid = K, block = 64 * hw.  LDS: G, G^T (2 n*n) | per wave: V_{l,j} (m Q (1+V) x 64) | per wave: m*m + m + 1 sums
// ---------------------------------------------------------------------------------------------------------------------------------------------
template <int V, int Q>
__global__ void __launch_bounds__(512) pcl_var_hess_kernel(VarParams p) {
    extern __shared__ double pcl_var_lds[];
    const int n = p.n, nn = n * n, C = p.cols, m = p.m, nw = p.hw;
    const int k = blockIdx.x;
    if (k >= p.K) return;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double *G = pcl_var_lds, *GT = G + nn;
    const int slab = m * Q * (V + 1) * 64, nsum = m * m + m + 1;
    double *Vs = GT + nn + (size_t)wave * slab;
    double *sums = GT + nn + (size_t)nw * slab;
    const double *z0 = p.Z + (size_t)k * p.z_dim, *z1 = z0 + p.z_dim;
    for (int e = threadIdx.x; e < nn; e += blockDim.x) {
        double a = p.G0[e], at = p.G0T[e];
        for (int l = 0; l < m; ++l) a = fma(z0[p.u_off + l], p.Gj[(size_t)l * nn + e], a), at = fma(z0[p.u_off + l], p.GjT[(size_t)l * nn + e], at);
        G[e] = a;
        GT[e] = at;
    }
    for (int e = threadIdx.x; e < nw * nsum; e += blockDim.x) sums[e] = 0.0;
    __syncthreads();
    const double h = z0[p.dt_off];
    double T[Q + 1], T1[Q + 1], T2[Q + 1];
    pcl_var_coeffs<Q>(p.c, h, T, T1, T2);
    const long long xdc = (long long)n * C, xdl = xdc * (V + 1);
    const bool on = lane < n;
    double *out = p.hess + (size_t)k * p.hper;
    const int s0 = m * (m + 1) / 2 + m + 1;  // first X entry
    double *sw = sums + (size_t)wave * nsum;
    for (int c = wave; c < C; c += nw) {
        double Ye[V + 1], Yo[V + 1], W[Q + 1][V + 1];
#pragma unroll
        for (int b = 0; b <= V; ++b) {
            const double x0 = on ? z0[p.xo[b] + (size_t)c * n + lane] : 0.0;
            const double x1 = on ? z1[p.xo[b] + (size_t)c * n + lane] : 0.0;
            Ye[b] = x1 - x0;
            Yo[b] = -x1 - x0;
            W[0][b] = on ? p.mu[(size_t)k * xdl + b * xdc + (size_t)c * n + lane] : 0.0;
        }
#pragma unroll
        for (int j = 1; j <= Q; ++j) pcl_var_adj<V>(GT, p.GvT, n, lane, W[j - 1], W[j]);
        // (h,h)
        {
            double a = 0.0;
#pragma unroll
            for (int j = 2; j <= Q; ++j)
#pragma unroll
                for (int b = 0; b <= V; ++b) a = fma(T2[j], W[j][b] * ((j & 1) ? Yo[b] : Ye[b]), a);
            a = pcl_var_wave_sum(a);
            if (lane == 0) sw[m * m + m] += a;
        }
        // d2/dh dX
        {
            double sk[V + 1], sn[V + 1];
#pragma unroll
            for (int b = 0; b <= V; ++b) sk[b] = 0.0, sn[b] = 0.0;
#pragma unroll
            for (int j = 1; j <= Q; ++j)
#pragma unroll
                for (int b = 0; b <= V; ++b) sk[b] = fma(-T1[j], W[j][b], sk[b]), sn[b] = fma((j & 1) ? -T1[j] : T1[j], W[j][b], sn[b]);
            if (on) {
#pragma unroll
                for (int b = 0; b <= V; ++b) {
                    const size_t r = b * xdc + (size_t)c * n + lane;
                    out[s0 + (size_t)m * xdl + r] = sk[b];
                    out[s0 + (size_t)(2 * m + 1) * xdl + r] = sn[b];  // seg 6, behind seg 5 (m x xdl)
                }
            }
        }
        // V_{l,j} -> LDS slab [(l*Q + j-1)*(V+1) + b][64]; (h,u_l); d2/du_l dX
        for (int l = 0; l < m; ++l) {
            const double *GlT = p.GjT + (size_t)l * nn;
            double Vc[V + 1], t[V + 1], s[V + 1];
            pcl_var_mv<V + 1>(GlT, n, lane, W[0], Vc);
            double hu = 0.0, sk[V + 1], sn[V + 1];
#pragma unroll
            for (int b = 0; b <= V; ++b) sk[b] = -T[1] * Vc[b], sn[b] = -T[1] * Vc[b], hu = fma(T1[1], Vc[b] * Yo[b], hu);
#pragma unroll
            for (int b = 0; b <= V; ++b) Vs[((l * Q + 0) * (V + 1) + b) * 64 + lane] = Vc[b];
#pragma unroll
            for (int j = 2; j <= Q; ++j) {
                pcl_var_adj<V>(GT, p.GvT, n, lane, Vc, t);
                pcl_var_mv<V + 1>(GlT, n, lane, W[j - 1], s);
#pragma unroll
                for (int b = 0; b <= V; ++b) {
                    Vc[b] = t[b] + s[b];
                    Vs[((l * Q + j - 1) * (V + 1) + b) * 64 + lane] = Vc[b];
                    sk[b] = fma(-T[j], Vc[b], sk[b]);
                    sn[b] = fma((j & 1) ? -T[j] : T[j], Vc[b], sn[b]);
                    hu = fma(T1[j], Vc[b] * ((j & 1) ? Yo[b] : Ye[b]), hu);
                }
            }
            hu = pcl_var_wave_sum(hu);
            if (lane == 0) sw[m * m + l] += hu;
            if (on) {
#pragma unroll
                for (int b = 0; b <= V; ++b) {
                    const size_t r = b * xdc + (size_t)c * n + lane;
                    out[s0 + (size_t)l * xdl + r] = sk[b];
                    out[s0 + (size_t)(m + 1) * xdl + (size_t)l * xdl + r] = sn[b];
                }
            }
        }
        // (u_i,u_l): R_e chain (e = 1 .. Q-1), S_{l,e} = Ghat_l R_e, Tm[i][l] = sum_e <V_{i,e}, S_{l,e}>
        if (Q >= 2) {
            double R[Q][V + 1], t[V + 1];
#pragma unroll
            for (int b = 0; b <= V; ++b) R[Q - 1][b] = T[Q] * ((Q & 1) ? Yo[b] : Ye[b]);
#pragma unroll
            for (int e = Q - 2; e >= 1; --e) {
                pcl_var_fwd<V>(G, p.Gv, n, lane, R[e + 1], t);
#pragma unroll
                for (int b = 0; b <= V; ++b) R[e][b] = fma(T[e + 1], ((e + 1) & 1) ? Yo[b] : Ye[b], t[b]);
            }
            for (int l = 0; l < m; ++l) {
                const double *Gl = p.Gj + (size_t)l * nn;
                double S[Q][V + 1];
#pragma unroll
                for (int e = 1; e < Q; ++e) pcl_var_mv<V + 1>(Gl, n, lane, R[e], S[e]);
                for (int i = 0; i < m; ++i) {
                    double a = 0.0;
#pragma unroll
                    for (int e = 1; e < Q; ++e)
#pragma unroll
                        for (int b = 0; b <= V; ++b) a = fma(Vs[((i * Q + e - 1) * (V + 1) + b) * 64 + lane], S[e][b], a);
                    a = pcl_var_wave_sum(a);
                    if (lane == 0) sw[i * m + l] += a;
                }
            }
        }
    }
    __syncthreads();
    // scalar entries: seg 0 (u_i,u_l) l <= i, seg 1 (h,u_l), seg 2 (h,h); summed over the waves in order
    for (int e = threadIdx.x; e < s0; e += blockDim.x) {
        double a = 0.0;
        if (e < m * (m + 1) / 2) {
            int i = 0;
            while ((i + 1) * (i + 2) / 2 <= e) ++i;
            const int l = e - i * (i + 1) / 2;
            for (int w = 0; w < nw; ++w) a += sums[(size_t)w * nsum + i * m + l] + sums[(size_t)w * nsum + l * m + i];
        } else if (e < m * (m + 1) / 2 + m) {
            const int l = e - m * (m + 1) / 2;
            for (int w = 0; w < nw; ++w) a += sums[(size_t)w * nsum + m * m + l];
        } else {
            for (int w = 0; w < nw; ++w) a += sums[(size_t)w * nsum + m * m + m];
        }
        out[e] = a;
    }
}
