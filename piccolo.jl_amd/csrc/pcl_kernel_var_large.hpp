// Large variational kernel (contexts created with PCL_BATCH_VARIATIONAL | PCL_LARGE_N | PCL_LARGE_VAR, 66 <= n <= 128): residual, and residual +
// Jacobian, of the variational (sensitivity) integrators at the diagonal Pade orders p = 2q (q <= 5).  Outputs, value order and layout are those of
// pcl_var_fused_kernel (pcl_kernel_variational.hpp) for the same system.
//
// The one-tile plan of pcl_kernel_pade_large.hpp carries over: the lifted generator var_G(G, [Gv_i]) is block lower triangular with G on the
// diagonal, so a lifted product is the same matrix-core product  G [columns]  on (1 + v) times as many columns, plus  Gv_b (the column of
// component 0)  on component b -- a sparse row product read from memory, the shape of the drive term.  The helpers are those of
// pcl_device_large.hpp: one wave per 16-row tile of G with its A operand in registers, fixed k order, four accumulators summed in one order, a wave-uniform
// mask from G alone, zero-filled LDS so that every operand load is unconditional.
//   - CHAIN unit (interval, state-column slice s of nc columns, drive group g of mg drives): per column and component b = 0 .. v
//         W_b    <- c_j Y_{b,j} + h (G W_b + [b > 0] Gv_b W_0)             V_b the same with j c_j (the last level without h: d delta / d dt)
//         dW_{b,l} <- h (G dW_{b,l} + [b > 0] Gv_b dW_{0,l} + G_l W_b)
//     Group 0 stores delta and the dt tails, every group the tails of its drives.  W and V are formed by every group with the same operations.
//     LDS (doubles): G | -S_b, D_b ((1 + v) nc each) | X ((1 + v) T nc) | X' | slack | us,  T = 2 + mg (W | V | dW_l ..; residual only: W alone).
//   - PANEL unit (interval, role r, npc columns of the powers): its own workgroups -- at n = 128 a chain unit of three components leaves no room for a
//     panel.  Role 0 carries P_j = G^j and accumulates B^{+-} = sum_j c_j (+-h)^j P_j, written to the 1 + v places it occurs in, `cols` copies each;
//     role i = 1 .. v carries P_j AND the Frechet powers Q_j^i = G Q_{j-1}^i + Gv_i P_{j-1} (Q_1^i = Gv_i) and accumulates L^{+-}_i =
//     sum_{j>=1} c_j (+-h)^j Q_j^i: one variation per unit, P recomputed with the same bits, so a thread holds PL_NP pairs of ONE accumulator pair.
//     LDS: G | P' (npc) | Q (npc) | Q' (npc) | slack | us: the panel of P rotates between P' and its own columns of G.
// Every element of every output is formed by one fixed sequence of operations whatever the split (sx, mg, npc): no atomics, no sum across units,
// no workgroup waits for another.  Component 0 (delta_0, its tails, -B+ | B-) goes through the operations of pcl_pade_large_kernel in its order:
// the bits of a plain PCL_LARGE_N context of the same drift and drives.
#pragma once

struct VarLargeParams {
    const double *Gv;       // the variation generators dense, [v][n * n] column-major (Q_1 of the panel role)
    const double *gv_val;   // ... and row-compressed, [v][n][gv_w] (row-major, zero padded, columns ascending): the Gv_b terms of both roles
    const int *gv_col;
    int gv_w;
    int v;
    int xo[1 + PCL_VAR_MAXV];  // state offsets of the components in the knot
    int sx, mg, ngrp;          // chain units: state-column slices, drives per group, groups
    int npc, pu;               // panel units: columns of the powers per unit, units per role
};

// p: Z, delta, jac, G0, upos / ucoef / n_upos (build_G), ell_* (the drives), n, cols, m, K, z_dim, u_off, dt_off, LD, nc, S = units per interval,
// q, pc, lds_doubles, jac_per, nt -- as launch_pade_large fills them
template <bool JAC>
__global__ __launch_bounds__(PL_NT) void pcl_var_large_kernel(const KParams p, const VarLargeParams w) {
    extern __shared__ double lds[];
    const int n = p.n, d = p.cols, m = p.m, LD = p.LD, nc = p.nc, q = p.q, U = p.S, v = w.v;
    const int tid = threadIdx.x, nth = blockDim.x, lane = tid & 63, rt = tid >> 6;  // one wave per row tile
    const int li = lane & 15, lk = lane >> 4;
    const long long bid = blockIdx.x;
    const long long k = bid / U;
    const int u = (int)(bid % U);
    const double *zk = p.Z + k * p.z_dim;
    const double *zn = zk + p.z_dim;
    const double h = zk[p.dt_off];
    const long long nn = (long long)n * n;
    const int nchain = w.sx * w.ngrp;
    const bool chain = u < nchain;
    double *G = lds;
    double *us = lds + p.lds_doubles - (m + 8);
    for (int e = tid; e < p.lds_doubles; e += nth) lds[e] = 0.0;
    __syncthreads();
    build_G(p, p.G0, zk, G, us);
    const int ew = p.ell_w, gw = w.gv_w;
    if (chain) {
        const int s = u % w.sx, g = u / w.sx, mg = w.mg;
        const int c0 = s * nc, nce = max(0, min(nc, d - c0));            // this unit's state columns
        const int l0 = g * mg, mge = JAC ? max(0, min(mg, m - l0)) : 0;  // ... and drives
        const int T = JAC ? 2 + mg : 1, LDc = LD * nc, CB = T * LDc;     // CB: the X blocks of one component
        double *Sm = G + LD * n, *Dm = Sm + (1 + v) * LDc, *Xc = Dm + (1 + v) * LDc, *Xn = Xc + (1 + v) * CB;
        const double cq = p.pc[q];
        for (int e = tid; e < (1 + v) * nce * n; e += nth) {  // (columns beyond nce and the dW blocks stay zero)
            const int b = e / (nce * n), r = e - b * nce * n, c = r / n, i = r - c * n;
            const long long off = w.xo[b] + (long long)(c0 + c) * n + i;
            const double xn = zn[off], xc = zk[off];
            const double xs = xn + xc, xdv = xn - xc;
            const int idx = i + LD * c;
            Sm[b * LDc + idx] = -xs;
            Dm[b * LDc + idx] = xdv;
            const double yq = (q & 1) ? -xs : xdv;
            Xc[b * CB + idx] = cq * yq;
            if (JAC) Xc[b * CB + LDc + idx] = (q * cq) * yq;
        }
        __syncthreads();
        double a[PL_KS];
        const unsigned kmask = pl_load_a<false>(G, LD, n, rt, li, lk, a);  // (from G alone, never from the split or from a Gv)
        const int cb = T * nc, cx = (1 + v) * cb, ct_n = (cx + 15) >> 4;
        for (int j = q - 1; j >= 0; --j) {
            const double *Yj = (j & 1) ? Sm : Dm;
            const double cj = p.pc[j];
            for (int ct = 0; ct < ct_n; ++ct) {
                const int vc = ct * 16 + li;
                const int b = min(vc / cb, v), rem = vc - b * cb, bl = rem / nc, c = rem - bl * nc;
                const bool on = vc < cx && c < nce && (bl < 2 || bl - 2 < mge);
                const double4_t acc = pl_tile(a, (on ? Xc + b * CB + bl * LDc + LD * c : G) + lk, kmask);
                if (on) {
                    // the additive terms of each element: c_j Y_j, j c_j Y_j, or the drive's sparse product with the old W_b; on a variation the
                    // sparse product of Gv_b with the old column of component 0.  Loads are unconditional (rows beyond n - 1 read finite padding
                    // or the last row; the stores below are predicated)
                    const int r0 = rt * 16 + lk;
                    double y[4] = {0.0, 0.0, 0.0, 0.0}, t[4];
                    if (bl <= 1) {
#pragma unroll
                        for (int r = 0; r < 4; ++r) y[r] = Yj[b * LDc + r0 + 4 * r + LD * c];
                    } else {
                        const double *wc = Xc + b * CB + LD * c;
                        const long long lrow = (long long)(l0 + bl - 2) * n;
#pragma unroll
                        for (int r = 0; r < 4; ++r) y[r] = pl_row_dot(p.ell_val, p.ell_col, (lrow + min(r0 + 4 * r, n - 1)) * ew, ew, wc);
                    }
#pragma unroll
                    for (int r = 0; r < 4; ++r) t[r] = acc[r];
                    if (b > 0) {
                        const double *x0 = Xc + bl * LDc + LD * c;  // the same block and column of component 0
                        const long long vrow = (long long)(b - 1) * n;
#pragma unroll
                        for (int r = 0; r < 4; ++r) t[r] = acc[r] + pl_row_dot(w.gv_val, w.gv_col, (vrow + min(r0 + 4 * r, n - 1)) * gw, gw, x0);
                    }
                    double *dst = Xn + b * CB + bl * LDc + LD * c;
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int rr = r0 + 4 * r;
                        double o;
                        if (bl == 0)
                            o = __builtin_fma(h, t[r], cj * y[r]);
                        else if (bl == 1)
                            o = j ? __builtin_fma(h, t[r], (j * cj) * y[r]) : t[r];
                        else
                            o = h * (t[r] + y[r]);
                        if (rr < n) dst[rr] = o;
                    }
                }
            }
            __syncthreads();  // level j is complete in X'; nothing reads X any more
            double *t_ = Xc;
            Xc = Xn;
            Xn = t_;
        }
        const long long xdc = (long long)n * d, xdl = xdc * (1 + v);
        if (p.delta && g == 0)
            for (int e = tid; e < (1 + v) * nce * n; e += nth) {
                const int b = e / (nce * n), r = e - b * nce * n, c = r / n, i = r - c * n;
                p.delta[k * xdl + b * xdc + (long long)(c0 + c) * n + i] = Xc[b * CB + i + LD * c];
            }
        if (!JAC) return;
        // tails [component][c][l | dt][i]: this group's drives, and the dt block from group 0
        double *jt = p.jac + k * p.jac_per + (2LL + 4LL * v) * d * nn;
        const int nl = mge + (g == 0 ? 1 : 0);
        for (int e = tid; e < (1 + v) * nl * nce * n; e += nth) {
            const int i = e % n, tt = (e / n) % nl, c = (e / (n * nl)) % nce, b = e / (n * nl * nce);
            const int l = tt < mge ? l0 + tt : m;
            jt[(((long long)b * d + c0 + c) * (m + 1) + l) * n + i] = Xc[b * CB + (tt < mge ? 2 + tt : 1) * LDc + i + LD * c];
        }
        return;
    }
    if (!JAC) return;
    // ---- panel unit: role 0 the powers and B^{+-}; role i the powers, the Frechet powers of variation i and L^{+-}_i ----
    const int pi = u - nchain, role = pi / w.pu, ps = pi - role * w.pu, npc = w.npc;
    const int pc0 = ps * npc, npce = max(0, min(npc, n - pc0));
    double *Pn = G + LD * n, *Qc = Pn + LD * npc, *Qn = Qc + LD * npc, *Pc = G + LD * (npce > 0 ? pc0 : 0);
    if (role > 0) {
        const double *gvd = w.Gv + (long long)(role - 1) * nn + (long long)pc0 * n;
        for (int e = tid; e < npce * n; e += nth) Qc[(e % n) + LD * (e / n)] = gvd[e];
    }
    __syncthreads();
    double a[PL_KS];
    const unsigned kmask = pl_load_a<false>(G, LD, n, rt, li, lk, a);
    // each thread owns the flat positions (2 pi, 2 pi + 1), pi = tid + nth r, of the unit's panel (n x npce, contiguous in memory; n is even: both
    // lie in one column); first terms I + c_1 (+-h) G (role 0), c_1 (+-h) Gv_i (role i)
    double bp[PL_NP][2], bm[PL_NP][2];
    int o_[PL_NP];
    double hp = h, hm = -h;
    const int ptot = n * npce;
    {
        const double *Ac = role ? Qc : Pc;
#pragma unroll
        for (int r = 0; r < PL_NP; ++r) {
            const int pos = 2 * (tid + nth * r);
            o_[r] = -1;
            bp[r][0] = bm[r][0] = bp[r][1] = bm[r][1] = 0.0;
            if (pos < ptot) {
                const int c = pos / n, i = pos - c * n, c1 = (pos + 1) / n, i1 = pos + 1 - c1 * n;
                o_[r] = i + LD * c;
                bp[r][0] = bm[r][0] = (!role && i == pc0 + c) ? 1.0 : 0.0;
                bp[r][1] = bm[r][1] = (!role && i1 == pc0 + c1) ? 1.0 : 0.0;
                const double v0 = Ac[o_[r]], v1 = Ac[o_[r] + 1];
                bp[r][0] += p.pc[1] * hp * v0;
                bp[r][1] += p.pc[1] * hp * v1;
                bm[r][0] += p.pc[1] * hm * v0;
                bm[r][1] += p.pc[1] * hm * v1;
            }
        }
    }
    const int cxp = role ? 2 * npc : npc, ct_n = (cxp + 15) >> 4;
    for (int j = q - 1; j >= 1; --j) {  // (the last level of the chains forms no power)
        for (int ct = 0; ct < ct_n; ++ct) {
            const int vc = ct * 16 + li;
            const bool isq = vc >= npc;  // a column of the Frechet powers
            const int c = isq ? vc - npc : vc;
            const bool on = vc < cxp && c < npce && (isq || !role || j > 1);  // (role i: the last power of G itself is not needed)
            const double4_t acc = pl_tile(a, (on ? (isq ? Qc : Pc) + LD * c : G) + lk, kmask);
            if (on) {
                const int r0 = rt * 16 + lk;
                double *dst = (isq ? Qn : Pn) + LD * c;
                const long long vrow = (long long)(role - 1) * n;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int rr = r0 + 4 * r;
                    double o = acc[r];
                    if (isq) o = acc[r] + pl_row_dot(w.gv_val, w.gv_col, (vrow + min(rr, n - 1)) * gw, gw, Pc + LD * c);
                    if (rr < n) dst[rr] = o;
                }
            }
        }
        __syncthreads();  // the next powers are complete in P' / Q'; nothing reads P / Q any more
        double *t_ = Pc;
        Pc = Pn;
        Pn = t_;
        t_ = Qc;
        Qc = Qn;
        Qn = t_;
        const int pw = q + 1 - j;
        const double *Ac = role ? Qc : Pc;
        hp *= h;
        hm *= -h;
#pragma unroll
        for (int r = 0; r < PL_NP; ++r)
            if (o_[r] >= 0) {
                const double v0 = Ac[o_[r]], v1 = Ac[o_[r] + 1];
                bp[r][0] += p.pc[pw] * hp * v0;
                bp[r][1] += p.pc[pw] * hp * v1;
                bm[r][0] += p.pc[pw] * hm * v0;
                bm[r][1] += p.pc[pw] * hm * v1;
            }
    }
    // role 0: -B^+ | B^- of delta_0 and of every variation; role i: -L^+_i | L^-_i -- this unit's panel, into every replicated position
    double *jb = p.jac + k * p.jac_per;
    const long long blk = (long long)d * nn;
    const int nplace = role ? 1 : 1 + v;
#pragma unroll
    for (int r = 0; r < PL_NP; ++r)
        if (o_[r] >= 0) {
            const int pos = 2 * (tid + nth * r);
            for (int pl = 0; pl < nplace; ++pl) {
                const long long seg = role ? 4LL * role : (pl ? 4LL * pl - 2 : 0);  // [-B+ B-] [-B+ B- -L+_1 L-_1] [-B+ B- -L+_2 L-_2]
                double *o0 = jb + seg * blk + (long long)pc0 * n + pos;
                for (int c = 0; c < d; ++c) {
                    store2(o0 + c * nn, -bp[r][0], -bp[r][1], p.nt);
                    store2(o0 + blk + c * nn, bm[r][0], bm[r][1], p.nt);
                }
            }
        }
}
