// Large exponential kernel (contexts created with PCL_LARGE_N | PCL_LARGE_EXP and pade_order = PCL_ORDER_EXP, 66 <= n <= 128): residual, and
// residual + exact Jacobian, of  delta_k = X_{k+1} - exp(dt_k G(u_k)) X_k.  Outputs, value order and layout are those of pcl_exp_kernel
// (pcl_kernel_exp.hpp) for the same KParams: per interval `cols` copies of -E, the diagonal ones of d delta / d X_{k+1}, then the tails
// [c][l | dt][i] = -L_l X_k | -G E X_k.
//
// Scaling and squaring needs three or more n x n tiles; ONE fits (LD = n | 1: 132,096 B of 163,840 B at n = 128).  Neither E nor the Frechet
// derivatives L_l are needed as matrices (but for the one -E block of the values), so the kernel is the SUBSTEPPED Taylor polynomial of
// pcl_kernel_large_rollout.hpp in action form, with the derivative carried through it.  s' = ceil(|h| |G|_1) substeps of h_s = h / s' (computed
// in the workgroup from the tile: every unit of an interval builds the same tile with the same operations, hence the same s'; at most LR_SMAX).
// Per substep, from Y (at first X_k) and dY_l (at first 0), Horner for j = LE_DEG .. 1 with f = h_s / j:
//       dV_l <- dY_l + f (G dV_l + G_l V)      (the V before this level's update)
//       V    <- Y + f G V
// then Y <- V, dY_l <- dV_l.  After the last substep delta = X_{k+1} - Y, the drive tails are -dY_l and the dt tail is -G Y (one more product);
// -E is the V recurrence on column panels of the identity.  h = 0: s' = 0, so E = I exactly, delta = X_{k+1} - X_k, zero drive tails and the dt
// tail -G X_k.  A negative h is an ordinary step.
//
// The plan is that of pcl_kernel_pade_large.hpp: one LDS tile for G(u_k), one wave per 16-row tile with its A operand in registers over the
// whole loop, v_mfma_f64_16x16x4_f64 through pl_tile, PL_SLACK doubles behind the last column block and zero-filled LDS so that every operand
// read is finite, the drives' ELL rows read through L2.  An interval is split into U units, one workgroup each.  Unit u < sx ngrp is a CHAIN
// unit: state-column slice s = u % sx (nc columns) and drive group g = u / sx (mg drives); it runs V and the dV_l of its drives (V is needed by
// every group and is formed by each with the same operations, hence the same bits).  Group 0 stores delta, the ones and the dt tail, every
// group the tails of its drives.  Every unit u with u npc < n also carries the PANEL of columns [u npc, (u + 1) npc) of E and stores it to all
// `cols` copies.  The left factors G and G_l are constant through the loop, so every column is independent: no sum crosses a unit.
// LDS (doubles): G | three buffers of W = nc (1 + mg) + npc columns (Y, V, the level's result; they rotate) | slack | us.
//
// Truncation.  With |h_s G|_1 <= 1 the value's remainder of the degree-18 polynomial is at most sum_{j >= 19} 1 / j! < 8.7e-18 per substep (2.4e-17
// of |exp(h_s G)| >= exp(-1), below 2^-53).  The derivative of the polynomial misses  sum_{j >= 19} d(A^j) / j!,  A = h_s G:  |d(A^j)| <= j |A|^{j-1} |dA|,
// so its remainder is at most  sum_{j >= 19} 1 / (j - 1)! = sum_{j >= 18} 1 / j! < 1.6e-16  of |h_s G_l| per substep -- again below 2^-53 of the
// term it belongs to.  Degree 17 would give 3.0e-15.  Beyond |h| |G|_1 = LR_SMAX the launch stays bounded and the result is that of the
// truncated series at a step that is too long; a NaN norm takes the clamp and gives NaN.
//
// Every element of every output is formed by one fixed sequence of operations whatever the split (sx, mg, npc): the k order of the products is
// pl_tile's, the additive terms are explicit fused multiply-adds -- no atomics, and every split gives the same bits; the residual-only launch
// runs V alone and gives the bits of the fused launch.  Odd n (PCL_STATE_VECTOR): the blocks are not 16-byte aligned; the stores are scalar.
//
// MODE (option large_exp_reduce; the plain launch is LE_FULL, the code it had before the modes -- they mirror pcl_kernel_pade_large.hpp):
//   LE_COMPACT  the compact Jacobian [-E (n n) | tails]: every unit stores its panel once instead of `cols` times, the ones of d delta / d X_{k+1}
//               are not written and the tails start behind n n; the same registers and operations, so the values and delta have the same bits;
//   LE_MERIT    the full values and, behind the last substep and the G Y product, the reduce payload's partial sums: a chain unit (slice s, group g)
//               forms, per state column of its slice, <d delta / d u_l, lam> for each of its drives (-dY_l in LDS), and group 0 also
//               <d delta / d dt, lam> (-G Y) and <lam, delta> (times 1/2 when lam = delta; delta is then staged in the free buffer) -- one wave per
//               (column, job), lane i takes rows i and i + 64 by fused multiply-adds in that order, then the shuffle tree: the order of the additions
//               depends on n alone.  Plain stores into p.mpart[((b K + k) cols + c)(m + 2) + l], which pcl_merit_finish_kernel reads; exactly one
//               unit owns each (c, l), panel-only units own nothing: no atomics, no sum across units, every split the same bits;
//   LE_PAYLOAD  delta and those partial sums alone (npc = 0, U = sx ngrp chain units): no identity panel, no block store, no tail store.
#pragma once

#define LE_DEG 18  // (the builder's choice; LR_DEG of the rollout, whose discretisation the rows then share)

// p.S = U units per interval, p.nc state columns per chain unit; sx state-column slices, mg drives per group, npc columns of E per unit
enum { LE_FULL = 0, LE_COMPACT = 1, LE_MERIT = 2, LE_PAYLOAD = 3 };
template <bool JAC, int MODE = LE_FULL>
__global__ __launch_bounds__(PL_NT) void pcl_large_exp_kernel(const KParams p, const int sx, const int mg, const int npc) {
    static_assert(JAC || MODE == LE_FULL, "the modes belong to the Jacobian launch");
    constexpr bool PANEL = JAC && MODE != LE_PAYLOAD;  // the panel of the identity: the columns of E
    extern __shared__ double lds[];
    const int n = p.n, d = p.cols, m = p.m, LD = p.LD, nc = p.nc, U = p.S;
    const int tid = threadIdx.x, nth = blockDim.x, lane = tid & 63, rt = tid >> 6;  // one wave per row tile
    const int li = lane & 15, lk = lane >> 4;
    const long long bid = blockIdx.x;
    const long long item = bid / U;
    const int u = (int)(bid % U);
    const int k = (int)(item % p.K), b = (int)(item / p.K);
    const double *zk = p.Z + (long long)b * p.z_batch_stride + (long long)k * p.z_dim;
    const double *zn = zk + p.z_dim;
    const double h = zk[p.dt_off];
    const long long nn = (long long)n * n;
    const int ngrp = (JAC && m > 0) ? (m + mg - 1) / mg : 1;
    const bool chain = u < sx * ngrp;
    const int s = chain ? u % sx : 0, g = chain ? u / sx : 0;
    const int c0 = s * nc, nce = chain ? max(0, min(nc, d - c0)) : 0;           // this unit's state columns
    const int l0 = g * mg, mge = (JAC && chain) ? max(0, min(mg, m - l0)) : 0;  // ... and drives
    const int T = JAC ? 1 + mg : 1;                                             // blocks per state column: V | dV_l0 ..
    const int W = T * nc + (PANEL ? npc : 0), cx = chain ? T * nc : 0;          // columns of a buffer; the chain's share of them
    const int pc0 = PANEL ? u * npc : n, npce = max(0, min(npc, n - pc0));        // ... and columns of E
    double *G = lds, *B0 = G + LD * n, *B1 = B0 + LD * W, *B2 = B1 + LD * W;
    double *us = B2 + LD * W + PL_SLACK;
    for (int e = tid; e < p.lds_doubles; e += nth) lds[e] = 0.0;
    __syncthreads();
    const int x_off = p.x_offs[p.z_batch_stride ? 0 : b];
    build_G(p, p.G0 + (long long)b * p.g0_batch_stride, zk, G, us);
    __syncthreads();
    // |G|_1: the column sums go through the third buffer (n <= LD W doubles; read back before anything else is written there)
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
    __syncthreads();  // (the norms have been read)
    if (tid < n) B2[tid] = 0.0;
    for (int e = tid; e < nce * n; e += nth) {  // Y = X_k; the dY blocks stay zero
        const int c = e / n, i = e - c * n;
        B0[i + LD * c] = zk[x_off + (c0 + c) * n + i];
    }
    for (int e = tid; e < npce * n; e += nth) {  // ... and the panel of the identity
        const int c = e / n, i = e - c * n;
        B0[i + LD * (cx + c)] = (i == pc0 + c) ? 1.0 : 0.0;
    }
    __syncthreads();
    double *Y = B0, *f1 = B1, *f2 = B2;
    const int ct_n = (cx + npce + 15) >> 4;
    const int ew = p.ell_w;
    for (int st = 0; st < sp; ++st) {
        double *V = Y, *D = f1, *O = f2;
        for (int j = LE_DEG; j >= 1; --j) {
            const double f = hs / j;
            for (int ct = 0; ct < ct_n; ++ct) {
                const int vc = ct * 16 + li;
                const bool isp = vc >= cx;  // a column of E
                const int bl = isp ? 0 : vc / nc, c = isp ? vc - cx : vc - bl * nc;
                const bool on = isp ? c < npce : (c < nce && (bl == 0 || bl - 1 < mge));
                const double4_t acc = pl_tile(a, (on ? V + LD * vc : G) + lk, kmask);
                if (on) {
                    const int r0 = rt * 16 + lk;
                    double y[4] = {0.0, 0.0, 0.0, 0.0};
                    if (JAC && !isp && bl > 0) {  // G_l V, with the V before this level's update
                        const double *wc = V + LD * c;
                        const long long lrow = (long long)(l0 + bl - 1) * n;
#pragma unroll
                        for (int r = 0; r < 4; ++r) y[r] = pl_row_dot(p.ell_val, p.ell_col, (lrow + min(r0 + 4 * r, n - 1)) * ew, ew, wc);
                    }
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int rr = r0 + 4 * r;
                        if (rr < n) D[rr + LD * vc] = __builtin_fma(f, (JAC && !isp && bl > 0) ? acc[r] + y[r] : acc[r], Y[rr + LD * vc]);
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
    const bool first = chain && g == 0;
    if (JAC && first) {  // the dt tail: G Y into the free buffer (the sign goes on with the store)
        for (int ct = 0; ct < (nce + 15) >> 4; ++ct) {
            const int vc = ct * 16 + li;
            const bool on = vc < nce;
            const double4_t acc = pl_tile(a, (on ? Y + LD * vc : G) + lk, kmask);
            if (on) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int rr = rt * 16 + lk + 4 * r;
                    if (rr < n) f1[rr + LD * vc] = acc[r];
                }
            }
        }
        __syncthreads();
    }
    const long long xd = (long long)n * d;
    if (p.delta && first)
        for (int e = tid; e < nce * n; e += nth) {
            const int c = e / n, i = e - c * n;
            p.delta[item * xd + (long long)c0 * n + e] = zn[x_off + (c0 + c) * n + i] - Y[i + LD * c];
        }
    if (!JAC) return;
    const int nl = mge + (first ? 1 : 0);
    if (MODE == LE_MERIT || MODE == LE_PAYLOAD) {
        // the payload's partial sums of this unit's columns: jobs t < mge its drives, then (group 0) dt and <lam, delta>; lam = delta is staged in the
        // free buffer by the expression of the store above
        const double *lamg = p.mlam ? p.mlam + item * xd + (long long)c0 * n : nullptr;
        if (!lamg) {
            for (int e = tid; e < nce * n; e += nth) {
                const int c = e / n, i = e - c * n;
                f2[i + LD * c] = zn[x_off + (c0 + c) * n + i] - Y[i + LD * c];
            }
            __syncthreads();
        }
        const int nj = nl + (first ? 1 : 0), nw = nth >> 6;
        for (int job = rt; job < nce * nj; job += nw) {
            const int c = job / nj, t = job - c * nj;
            const double *x = t < mge ? Y + LD * ((1 + t) * nc + c) : f1 + LD * c;  // dY_l | G Y: the tails are their negatives
            const double *lm = lamg ? lamg + c * n : f2 + LD * c;
            double sacc = 0.0;
            if (t <= mge) {
                for (int i = lane; i < n; i += 64) sacc = __builtin_fma(-x[i], lm[i], sacc);
            } else if (lamg) {
                for (int i = lane; i < n; i += 64) sacc = __builtin_fma(zn[x_off + (c0 + c) * n + i] - Y[i + LD * c], lm[i], sacc);
            } else {
                for (int i = lane; i < n; i += 64) sacc = __builtin_fma(lm[i], lm[i], sacc);
            }
            sacc = wave_sum(sacc);
            if (t == mge + 1 && !lamg) sacc *= 0.5;
            if (lane == 0) p.mpart[(item * d + c0 + c) * (m + 2) + (t < mge ? l0 + t : m + (t - mge))] = sacc;
        }
        if (MODE == LE_PAYLOAD) return;
    }
    double *jb = p.jac + item * p.jac_per;
    const int dcp = MODE == LE_COMPACT ? 1 : d;  // copies of -E in the layout
    // d delta / d X_{k+1} = I: its diagonal, from the unit that has the column (not part of the compact layout)
    if (MODE != LE_COMPACT && first)
        for (int e = tid; e < nce * n; e += nth) jb[d * nn + (long long)c0 * n + e] = 1.0;
    // tails [c][l | dt][i]: this group's drives, and the dt block from group 0
    double *jt = jb + dcp * nn + (MODE == LE_COMPACT ? 0 : xd);
    for (int e = tid; e < nl * nce * n; e += nth) {
        const int i = e % n, t = (e / n) % nl, c = e / (n * nl);
        const int l = t < mge ? l0 + t : m;
        const double v = t < mge ? Y[i + LD * ((1 + t) * nc + c)] : f1[i + LD * c];
        jt[((long long)(c0 + c) * (m + 1) + l) * n + i] = -v;
    }
    // -E: this unit's panel, into every replicated position
    if (npce > 0) {
        const double *src = Y + LD * cx;
        double *o0 = jb + (long long)pc0 * n;
        if (!(n & 1) && !(reinterpret_cast<unsigned long long>(o0) & 15ull)) {
            const int hn = n >> 1;
            for (int e = tid; e < npce * hn; e += nth) {
                const int c = e / hn, i = 2 * (e - c * hn);
                const double v0 = -src[i + LD * c], v1 = -src[i + 1 + LD * c];
                for (int cc = 0; cc < dcp; ++cc) store2(o0 + cc * nn + c * n + i, v0, v1, p.nt);
            }
        } else {
            for (int e = tid; e < npce * n; e += nth) {
                const double v = -src[(e % n) + LD * (e / n)];
                for (int cc = 0; cc < dcp; ++cc) o0[cc * nn + e] = v;
            }
        }
    }
}
