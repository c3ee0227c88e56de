// Rollout on a large context (PCL_LARGE_N, 66 <= n <= 128; option large_full): X_{k+1} = exp(dt_k G(u_k)) X_k from the knot-0 state, output
// [batch][N][x_dim] -- the contract of pcl_expm_kernel + pcl_chain_kernel (pcl_kernels_misc.hpp).  Their scaling and squaring needs three n x n
// tiles; here ONE fits (LD = n | 1: 132,096 B of 163,840 B at n = 128).  So the propagator is a SUBSTEPPED Taylor polynomial, whose columns
// are independent under the constant left factor G, and the work is two launches on the LDS plan of pcl_kernel_pade_large.hpp (one wave per
// 16-row tile of G, the wave's A operand in registers over every product, v_mfma_f64_16x16x4_f64 through pl_tile, PL_SLACK doubles behind the
// last column block so that every B operand read is legal).
//
//   pcl_large_expm_kernel   one workgroup per (member, interval, panel of npc columns of E):
//       E[:, panel] = T(h_s G)^{s'} I[:, panel],   T(A) = sum_{j <= LR_DEG} A^j / j!  in Horner form  V <- Y + (h_s / j) G V,  j = LR_DEG .. 1,
//       s' = ceil(|h| |G|_1 / LR_THETA) substeps of h_s = h / s'.  s' is computed in the workgroup from the tile: every panel of an interval
//       builds the same tile with the same operations, hence the same s'.  h = 0: s' = 0 and E = I exactly; a negative h is an ordinary step.
//       LDS (doubles): G | three blocks of npc columns (Y, V, the product) | slack | us.  The panel goes to the context's workspace
//       [member][interval][n x n column-major].
//   pcl_large_chain_kernel  one workgroup per (member, slice of nc state columns): for k = 0 .. K - 1 the wave's A operand -- its 16 rows of
//       E_k -- goes from the workspace (L2) straight into registers, one interval ahead of the product that uses it, then one n x n x nc
//       product, knot k + 1 stored; one barrier per knot.  LDS: two blocks of nc columns | slack -- E_k itself never passes through LDS
//       (staging it in the tile and reading the operand back cost two more barriers and a round trip per knot: 9.6 us per knot at n = 96).
//
// Truncation.  With |h_s G|_1 <= LR_THETA = 1 the remainder of the degree-18 polynomial is at most sum_{j >= 19} 1 / j! < 1.06 / 19! =
// 8.7e-18; relative to |exp(h_s G)| >= exp(-1) that is 2.4e-17 < 2^-53 = 1.11e-16 (for the skew-symmetric iso generators |exp| = 1 and the
// margin is 13 x).  Degree 17 would give 4.5e-16.
// The clamp.  s' is at most LR_SMAX = 1024 (pcl_expm_kernel stops at 60 squarings in the same spirit): beyond |h| |G|_1 = 1024 -- no control
// problem is there -- the launch stays bounded (1024 x 18 products) and the result is that of the truncated series at a step that is too long.
// A NaN norm takes the clamp and gives NaN.
//
// Every element of every output is formed by one fixed sequence of operations whatever the split (panels, slices): a column's Horner chain
// never sees its neighbours, the k order of the products is pl_tile's, and no sum crosses a workgroup -- no atomics, the same bits.
// Odd n (PCL_STATE_VECTOR): panels and knots are not 16-byte aligned in memory; the stores are then scalar, as in the Jacobian kernel.
#pragma once

#define LR_DEG 18
#define LR_THETA 1.0
#define LR_SMAX 1024

// p.S = panels per interval, p.nc = columns of E per panel, p.lds_doubles = doubles of LDS to zero at the start
__global__ __launch_bounds__(PL_NT) void pcl_large_expm_kernel(const KParams p) {
    extern __shared__ double lds[];
    const int n = p.n, LD = p.LD, npc = p.nc, P = p.S;
    const int tid = threadIdx.x, nth = blockDim.x, lane = tid & 63, rt = tid >> 6;
    const int li = lane & 15, lk = lane >> 4;
    const long long bid = blockIdx.x, item = bid / P;
    const int u = (int)(bid % P);
    const int k = (int)(item % p.K), b = (int)(item / p.K);
    const double *zk = p.Z + (long long)b * p.z_batch_stride + (long long)k * p.z_dim;
    const double h = zk[p.dt_off];
    const int pc0 = u * npc, npce = max(0, min(npc, n - pc0));
    double *G = lds, *B0 = G + LD * n, *B1 = B0 + LD * npc, *B2 = B1 + LD * npc;
    double *us = B2 + LD * npc + PL_SLACK;
    for (int e = tid; e < p.lds_doubles; e += nth) lds[e] = 0.0;
    __syncthreads();
    build_G(p, p.G0 + (long long)b * p.g0_batch_stride, zk, G, us);
    __syncthreads();
    // |G|_1: the column sums go through the product block (n <= LD npc doubles; finite, and overwritten or never used as a nonzero operand)
    if (tid < n) {
        double cs = 0.0;
        for (int i = 0; i < n; ++i) cs += fabs(G[i + LD * tid]);
        B2[tid] = cs;
    }
    __syncthreads();
    double nrm = 0.0;
    for (int j = 0; j < n; ++j) nrm = fmax(nrm, B2[j]);
    const double x = fabs(h) * nrm;
    const int sp = x == 0.0 ? 0 : (x <= (double)LR_SMAX * LR_THETA ? (int)ceil(x / LR_THETA) : LR_SMAX);
    const double hs = sp > 0 ? h / sp : 0.0;
    double a[PL_KS];
    const unsigned kmask = pl_load_a<false>(G, LD, n, rt, li, lk, a);
    __syncthreads();  // (the norms have been read: the product block is free)
    for (int e = tid; e < npce * n; e += nth) {
        const int c = e / n, i = e - c * n;
        B0[i + LD * c] = (i == pc0 + c) ? 1.0 : 0.0;
    }
    __syncthreads();
    double *Y = B0, *f1 = B1, *f2 = B2;
    const int ct_n = (npce + 15) >> 4;
    for (int s = 0; s < sp; ++s) {
        double *V = Y, *D = f1, *O = f2;
        for (int j = LR_DEG; j >= 1; --j) {
            const double f = hs / j;
            for (int ct = 0; ct < ct_n; ++ct) {
                const int vc = ct * 16 + li;
                const bool on = vc < npce;
                const double4_t acc = pl_tile(a, (on ? V + LD * vc : G) + lk, kmask);
                if (on) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int rr = rt * 16 + lk + 4 * r;
                        if (rr < n) D[rr + LD * vc] = __builtin_fma(f, acc[r], Y[rr + LD * vc]);
                    }
                }
            }
            __syncthreads();  // level j is complete in D; nothing reads V any more
            if (V == Y) {
                V = D;
                D = O;
            } else {
                double *t_ = V;
                V = D;
                D = t_;
            }
        }
        f1 = D;
        f2 = Y;
        Y = V;
    }
    pl_store_cols(p.expm + item * (long long)n * n + (long long)pc0 * n, Y, n, LD, npce, tid, nth);
}

// pl_load_a's operand from memory, without the mask (E: n x n column-major, the workspace, read through L2): 16 consecutive rows per k-step
// and quarter wave, 128 B each
__device__ __forceinline__ void lr_fetch_a(const double *__restrict__ E, int n, int rt, int li, int lk, double (&a)[PL_KS]) {
#pragma unroll
    for (int ks = 0; ks < PL_KS; ++ks) {
        const int row = rt * 16 + li, kk = 4 * ks + lk;
        a[ks] = (row < n && kk < n) ? E[row + (long long)n * kk] : 0.0;
    }
}

// p.S = slices per member, p.nc = state columns per slice
__global__ __launch_bounds__(PL_NT) void pcl_large_chain_kernel(const KParams p) {
    extern __shared__ double lds[];
    const int n = p.n, LD = p.LD, nc = p.nc, S = p.S;
    const int tid = threadIdx.x, nth = blockDim.x, lane = tid & 63, rt = tid >> 6;
    const int li = lane & 15, lk = lane >> 4;
    const int b = (int)(blockIdx.x / S), s = (int)(blockIdx.x % S);
    const int c0 = s * nc, nce = max(0, min(nc, p.cols - c0));
    const long long xd = (long long)n * p.cols, nn = (long long)n * n;
    double *Xa = lds, *Xb = Xa + LD * nc;
    const double *Eb = p.expm + (long long)b * p.K * nn;
    double an[PL_KS];
    lr_fetch_a(Eb, n, rt, li, lk, an);  // (in flight while the state is loaded)
    for (int e = tid; e < p.lds_doubles; e += nth) lds[e] = 0.0;
    __syncthreads();
    const double *x0 = p.Z + (long long)b * p.z_batch_stride + p.x_offs[p.z_batch_stride ? 0 : b] + (long long)c0 * n;
    double *out = p.xout + (long long)b * (p.K + 1) * xd + (long long)c0 * n;
    for (int e = tid; e < nce * n; e += nth) {
        const double v = x0[e];
        Xa[(e % n) + LD * (e / n)] = v;
        out[e] = v;
    }
    __syncthreads();
    const int ct_n = (nce + 15) >> 4;
    double *cur = Xa, *oth = Xb;
    for (int k = 0; k < p.K; ++k) {
        double a[PL_KS];
        unsigned kmask = 0;
#pragma unroll
        for (int ks = 0; ks < PL_KS; ++ks) {
            a[ks] = an[ks];
            if (__ballot(a[ks] != 0.0)) kmask |= 1u << ks;
        }
        kmask = __builtin_amdgcn_readfirstlane(kmask);
        if (k + 1 < p.K) lr_fetch_a(Eb + (long long)(k + 1) * nn, n, rt, li, lk, an);  // the next interval's operand: in flight during this product
        for (int ct = 0; ct < ct_n; ++ct) {
            const int vc = ct * 16 + li;
            const bool on = vc < nce;
            const double4_t acc = pl_tile(a, cur + (on ? LD * vc : 0) + lk, kmask);
            if (on) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int rr = rt * 16 + lk + 4 * r;
                    if (rr < n) oth[rr + LD * vc] = acc[r];
                }
            }
        }
        __syncthreads();  // knot k + 1 is complete in `oth`; nothing reads `cur` any more (the next product writes it)
        pl_store_cols(out + (long long)(k + 1) * xd, oth, n, LD, nce, tid, nth);
        double *t_ = cur;
        cur = oth;
        oth = t_;
    }
}
