// Large-generator kernel (contexts created with PCL_LARGE_N, 66 <= n <= 128): residual, and residual + Jacobian, for the diagonal Pade orders
// p = 2q (q <= 5).  Outputs, value order and layout are those of pcl_pade_kernel<JAC> (pcl_kernels_reference.hpp) for the same KParams.
//
// The formulation is the lock-step one of pcl_kernel_pade_v2.hpp -- per level ONE product  G [W | V | dW_l .. | P]  on the matrix cores, the
// three Horner recursions and the panel of the powers of G side by side -- with the fixed counts of n <= 64 taken out:
//   - ONE n x n tile in LDS (LD = n | 1: 132,096 B at n = 128) and what is left of the 163,840 B in column blocks of LD doubles (29 at n = 128);
//   - one wave per 16-row tile of G (blockDim = 64 ceil(n / 16): 5 .. 8 waves, at most 2 per SIMD, so 256 registers per lane): the wave's
//     A operand, 32 k-steps, stays in registers over all levels (64 registers); the B operand is read 16 k-steps at a time;
//   - an interval is split into U units, one workgroup each.  Unit u < sx ngrp is a CHAIN unit: state-column slice s = u % sx (nc columns)
//     and drive group g = u / sx (mg drives): it runs W, V and the dW_l of its drives (W is needed by every group and is formed by each
//     with the same operations, hence the same bits).  Group 0 stores delta and the dt tail, every group the tails of its drives.  Every
//     unit u with u npc < n also carries the PANEL of columns [u npc, (u + 1) npc) of the powers of G, accumulates that panel of B^{+-} in
//     registers (PL_NP pairs per thread) and writes it to all `cols` copies;
//   - odd n (PCL_STATE_VECTOR): LD = n, so the panel is contiguous in LDS as it is in memory and a thread's pair may straddle two columns;
//     the block stores are then scalar (the blocks are not 16-byte aligned).
// LDS (doubles): G | -S | D | X (T nc) | X' (T nc) | P' (npc) | slack | us      T = 2 + mg blocks per state column (JAC), 1 (residual only).
// After the A operands are in registers nothing reads G as a matrix again: the panel rotates between P' and its own columns of G.
// Every element of every output is formed by one fixed sequence of operations whatever the split (sx, mg, npc): the k order of the products
// is fixed, the additive terms are explicit fused multiply-adds, and no sum crosses a unit -- no atomics, and every split gives the same bits.
// The drives' ELL rows are read from memory (L2): at m = 24, n = 120 they are 69 KB.
//
// MODE (option large_reduce; the plain launch is PL_FULL, the code it had before the modes):
//   PL_COMPACT  the compact Jacobian [-B+ | B- | tails]: every unit stores its panel once instead of `cols` times; the same registers, the same bits;
//   PL_MERIT    the full values and, once the level loop has ended, the reduce payload's partial sums: a chain unit (slice s, group g) forms, per
//               state column of its slice, <d delta / d u_l, lam> for each of its drives, and group 0 also <d delta / d dt, lam> and <lam, delta>
//               (times 1/2 when lam = delta) -- one wave per (column, job), lane-strided over the n rows, then the shuffle tree: the order of the
//               additions depends on n alone.  Plain stores into p.mpart[((b K + k) cols + c)(m + 2) + l], which pcl_merit_finish_kernel reads;
//               exactly one unit owns each (c, l): no atomics, no sum across units, every split the same bits;
//   PL_PAYLOAD  delta and those partial sums alone (npc = 0, U = sx ngrp chain units): no panel of the powers, no P' block, no block or tail store.
#pragma once

enum { PL_FULL = 0, PL_COMPACT = 1, PL_MERIT = 2, PL_PAYLOAD = 3 };

// p.S = U units per interval, p.nc state columns per chain unit; sx state-column slices, mg drives per group, npc power columns per unit
template <bool JAC, int MODE = PL_FULL>
__global__ __launch_bounds__(PL_NT) void pcl_pade_large_kernel(const KParams p, const int sx, const int mg, const int npc) {
    static_assert(JAC || MODE == PL_FULL, "the modes belong to the Jacobian launch");
    constexpr bool PANEL = JAC && MODE != PL_PAYLOAD;  // the panel of the powers and of B^{+-}
    extern __shared__ double lds[];
    const int n = p.n, d = p.cols, m = p.m, LD = p.LD, nc = p.nc, q = p.q, U = p.S;
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
    const int T = JAC ? 2 + mg : 1, LDc = LD * nc;
    const int pc0 = PANEL ? u * npc : n, npce = max(0, min(npc, n - pc0));      // ... and columns of the powers
    double *G = lds;
    double *Sm = G + LD * n, *Dm = Sm + LDc, *Xc = Dm + LDc, *Xn = Xc + T * LDc;  // X: W | V | dW_l0 .. (JAC), W alone otherwise
    double *Pn = Xn + T * LDc, *Pc = G + LD * (npce > 0 ? pc0 : 0);
    double *us = Pn + (PANEL ? LD * npc : 0) + PL_SLACK;
    for (int e = tid; e < p.lds_doubles; e += nth) lds[e] = 0.0;
    __syncthreads();
    const int x_off = p.x_offs[p.z_batch_stride ? 0 : b];
    build_G(p, p.G0 + (long long)b * p.g0_batch_stride, zk, G, us);
    const double cq = p.pc[q];
    for (int e = tid; e < nce * n; e += nth) {  // (columns beyond nce and the dW blocks stay zero)
        const int c = e / n, i = e - c * n;
        const double xn = zn[x_off + (c0 + c) * n + i], xc = zk[x_off + (c0 + c) * n + i];
        const double xs = xn + xc, xdv = xn - xc;
        const int idx = i + LD * c;
        Sm[idx] = -xs;
        Dm[idx] = xdv;
        const double yq = (q & 1) ? -xs : xdv;
        Xc[idx] = cq * yq;
        if (JAC) Xc[LDc + idx] = (q * cq) * yq;
    }
    __syncthreads();
    double a[PL_KS];
    const unsigned kmask = pl_load_a<false>(G, LD, n, rt, li, lk, a);
    // B^{+-}: each thread owns the flat positions (2 pi, 2 pi + 1), pi = tid + nth r, of the unit's panel (n x npce, contiguous in memory;
    // in LDS too when n is odd, LD = n; for an even n both positions lie in one column); first terms I + c_1 (+-h) G.  (This loop and the
    // per-level one below are the same text as pcl_var_large_kernel's on purpose: as shared helpers they cost this kernel's merit instance SGPR
    // spill reloads and time -- see pcl_device_large.hpp)
    double bp[PL_NP][2], bm[PL_NP][2];
    int o_[PL_NP];
    double hp = h, hm = -h;
    const int ptot = n * npce;
    if (PANEL) {
#pragma unroll
        for (int r = 0; r < PL_NP; ++r) {
            const int pos = 2 * (tid + nth * r);
            o_[r] = -1;
            bp[r][0] = bm[r][0] = bp[r][1] = bm[r][1] = 0.0;
            if (pos < ptot) {
                const int c = pos / n, i = pos - c * n, c1 = (pos + 1) / n, i1 = pos + 1 - c1 * n;
                o_[r] = i + LD * c;
                bp[r][0] = bm[r][0] = (i == pc0 + c) ? 1.0 : 0.0;
                bp[r][1] = bm[r][1] = (i1 == pc0 + c1) ? 1.0 : 0.0;
                const double v0 = Pc[o_[r]], v1 = Pc[o_[r] + 1];  // (the last position of an odd panel has no partner: finite padding, never stored)
                bp[r][0] += p.pc[1] * hp * v0;
                bp[r][1] += p.pc[1] * hp * v1;
                bm[r][0] += p.pc[1] * hm * v0;
                bm[r][1] += p.pc[1] * hm * v1;
            }
        }
    }
    const int cx = chain ? T * nc : 0, ct_n = (cx + (PANEL ? npc : 0) + 15) >> 4;
    const int ew = p.ell_w;
    for (int j = q - 1; j >= 0; --j) {
        const double *Yj = (j & 1) ? Sm : Dm;
        const double cj = p.pc[j];
        for (int ct = 0; ct < ct_n; ++ct) {
            if (j == 0 && ct * 16 >= cx) break;  // the last level forms no power
            const int vc = ct * 16 + li;
            const bool isp = vc >= cx;  // a column of the powers
            const int bl = isp ? T : vc / nc, c = isp ? vc - cx : vc - bl * nc;
            const bool on = isp ? (j > 0 && c < npce) : (c < nce && (bl < 2 || bl - 2 < mge));
            const double4_t acc = pl_tile(a, (on ? (isp ? Pc : Xc + bl * LDc) + LD * c : G) + lk, kmask);
            if (on) {
                // the additive term of each element: c_j Y_j, j c_j Y_j, or the drive's sparse product with the old W.  Loads are unconditional
                // (rows beyond n - 1 read finite padding; the stores below are predicated)
                const int r0 = rt * 16 + lk;
                double y[4] = {0.0, 0.0, 0.0, 0.0};
                if (bl <= 1) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) y[r] = Yj[r0 + 4 * r + LD * c];
                } else if (!isp) {
                    const double *wc = Xc + LD * c;
                    const long long lrow = (long long)(l0 + bl - 2) * n;
#pragma unroll
                    for (int r = 0; r < 4; ++r) y[r] = pl_row_dot(p.ell_val, p.ell_col, (lrow + min(r0 + 4 * r, n - 1)) * ew, ew, wc);
                }
                double *dst = (isp ? Pn : Xn + bl * LDc) + LD * c;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int rr = r0 + 4 * r;
                    double o;
                    if (bl == 0)
                        o = __builtin_fma(h, acc[r], cj * y[r]);
                    else if (bl == 1)
                        o = j ? __builtin_fma(h, acc[r], (j * cj) * y[r]) : acc[r];
                    else if (!isp)
                        o = h * (acc[r] + y[r]);
                    else
                        o = acc[r];
                    if (rr < n) dst[rr] = o;
                }
            }
        }
        __syncthreads();  // level j is complete in X' / P'; nothing reads X / P any more
        double *t_ = Xc;
        Xc = Xn;
        Xn = t_;
        if (PANEL && j > 0) {  // the next power: its term of B^{+-}
            t_ = Pc;
            Pc = Pn;
            Pn = t_;
            const int pw = q + 1 - j;
            hp *= h;
            hm *= -h;
#pragma unroll
            for (int r = 0; r < PL_NP; ++r)
                if (o_[r] >= 0) {
                    const double v0 = Pc[o_[r]], v1 = Pc[o_[r] + 1];
                    bp[r][0] += p.pc[pw] * hp * v0;
                    bp[r][1] += p.pc[pw] * hp * v1;
                    bm[r][0] += p.pc[pw] * hm * v0;
                    bm[r][1] += p.pc[pw] * hm * v1;
                }
        }
    }
    const long long xd = (long long)n * d;
    if (p.delta && g == 0)
        for (int e = tid; e < nce * n; e += nth) p.delta[item * xd + (long long)c0 * n + e] = Xc[(e % n) + LD * (e / n)];
    if (!JAC) return;
    const int nl = mge + (g == 0 ? 1 : 0);
    if (MODE == PL_MERIT || MODE == PL_PAYLOAD) {
        // the payload's partial sums of this unit's columns: jobs t < mge its drives, then (group 0) dt and <lam, delta>; lam = delta is read from W in LDS
        const int nj = nl + (g == 0 ? 1 : 0), nw = nth >> 6;
        const double *lamg = p.mlam ? p.mlam + item * xd + (long long)c0 * n : nullptr;
        for (int job = rt; job < nce * nj; job += nw) {
            const int c = job / nj, t = job - c * nj;
            const double *x = Xc + (t < mge ? 2 + t : (t == mge ? 1 : 0)) * LDc + LD * c;
            double sacc = 0.0;
            for (int i = lane; i < n; i += 64) sacc = __builtin_fma(x[i], lamg ? lamg[c * n + i] : Xc[i + LD * c], sacc);
            sacc = wave_sum(sacc);
            if (t == mge + 1 && !lamg) sacc *= 0.5;
            if (lane == 0) p.mpart[(item * d + c0 + c) * (m + 2) + (t < mge ? l0 + t : m + (t - mge))] = sacc;
        }
        if (MODE == PL_PAYLOAD) return;
    }
    double *jb = p.jac + item * p.jac_per;
    const int dcp = MODE == PL_COMPACT ? 1 : d;  // copies of a block in the layout
    const long long blk = (long long)dcp * nn;
    // tails [c][l | dt][i]: this group's drives, and the dt block from group 0
    double *jt = jb + 2 * blk;
    for (int e = tid; e < nl * nce * n; e += nth) {
        const int i = e % n, t = (e / n) % nl, c = e / (n * nl);
        const int l = t < mge ? l0 + t : m;
        jt[((long long)(c0 + c) * (m + 1) + l) * n + i] = Xc[(t < mge ? 2 + t : 1) * LDc + i + LD * c];
    }
    // -B^+ and B^-: this unit's panel, into every replicated position
    const bool even = !(n & 1);
#pragma unroll
    for (int r = 0; r < PL_NP; ++r)
        if (o_[r] >= 0) {
            const int pos = 2 * (tid + nth * r);
            double *o0 = jb + (long long)pc0 * n + pos;
            for (int c = 0; c < dcp; ++c) {
                if (even) {
                    store2(o0 + c * nn, -bp[r][0], -bp[r][1], p.nt);
                    store2(o0 + blk + c * nn, bm[r][0], bm[r][1], p.nt);
                } else {
                    o0[c * nn] = -bp[r][0];
                    o0[blk + c * nn] = bm[r][0];
                    if (pos + 1 < ptot) {
                        o0[c * nn + 1] = -bp[r][1];
                        o0[blk + c * nn + 1] = bm[r][1];
                    }
                }
            }
        }
}
