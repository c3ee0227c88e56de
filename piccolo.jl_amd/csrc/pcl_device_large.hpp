// What the large-generator kernels (66 <= n <= 128: pcl_kernel_pade_large*.hpp, pcl_kernel_large_*.hpp, pcl_kernel_var_large*.hpp) share: ONE n x n
// tile of G in LDS with LD = n | 1, one wave per 16-row tile of it with the wave's MFMA A operand in registers, zero-filled LDS and PL_SLACK doubles
// behind the last column block so that every B operand load is unconditional.  Each building block of that scheme has its one definition here;
// every kernel keeps its own LDS layout, level loop and stores.  The family's guarantee -- every element is formed by one fixed sequence of
// operations, so every split gives the same bits -- rests on these definitions: the k order of a product is pl_tile's, the order of a sparse row
// product is pl_row_dot's.  No helper knows which kernel calls it.  The B^{+-} panel registers of pcl_pade_large_kernel and pcl_var_large_kernel
// are NOT here: written as helpers, the init and the per-level accumulation changed the register allocation of pcl_pade_large_kernel (more SGPR
// spill reloads in the merit instance, which measured slower), so both kernels keep those two loops in place.
#pragma once

#define PL_KS 32     // k-steps of 4 (n <= 128)
#define PL_NT 512    // most threads per workgroup (8 row tiles)
#define PL_NP 8      // B^{+-} value pairs per thread (the host keeps n npc / 2 <= PL_NP blockDim)
#define PL_SLACK 128 // doubles behind the last column block: the B operand loads of a column run 128 rows whatever n is

// one 16 x 16 tile of G * B: a[] = this wave's rows of G, Bp = this lane's column of B in LDS + (lane >> 4), kmask = the k-steps with a nonzero
// in the wave's rows (wave-uniform).  Operand loads are unconditional, base + immediate: every double of the workgroup's LDS is finite
// (zero-filled at the start), and where k >= n the A operand is an exact zero
__device__ __forceinline__ double4_t pl_tile(const double (&a)[PL_KS], const double *__restrict__ Bp, unsigned kmask) {
    // k-step ks into accumulator ks mod 4: four independent chains (a dependent f64 MFMA waits for its accumulator), summed in one fixed order
    double4_t acc[4] = {{0.0, 0.0, 0.0, 0.0}, {0.0, 0.0, 0.0, 0.0}, {0.0, 0.0, 0.0, 0.0}, {0.0, 0.0, 0.0, 0.0}};
#pragma unroll
    for (int half = 0; half < 2; ++half) {
        double b[PL_KS / 2];
#pragma unroll
        for (int ks = 0; ks < PL_KS / 2; ++ks) b[ks] = Bp[4 * (ks + half * (PL_KS / 2))];
#pragma unroll
        for (int ks = 0; ks < PL_KS / 2; ++ks)
            if (kmask & (1u << (ks + half * (PL_KS / 2))))
                acc[ks & 3] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[ks + half * (PL_KS / 2)], b[ks], acc[ks & 3], 0, 0, 0);
    }
    return (acc[0] + acc[1]) + (acc[2] + acc[3]);
}

// the wave's 16 rows of the tile G (TRANSPOSED: of G^T, the tile's columns), 32 k-steps, into a[]; returns the k-steps with a nonzero among them
// (wave-uniform).  16 x 4 blocks without a nonzero are skipped by pl_tile (a dispersive qubit-cavity generator has a handful per row tile): adding
// their exact-zero products changes nothing but the sign of a zero sum.  The mask depends on the tile alone, never on the split
template <bool TRANSPOSED>
__device__ __forceinline__ unsigned pl_load_a(const double *__restrict__ G, int LD, int n, int rt, int li, int lk, double (&a)[PL_KS]) {
#pragma unroll
    for (int ks = 0; ks < PL_KS; ++ks) {
        const int row = rt * 16 + li, kk = 4 * ks + lk;
        a[ks] = (row < n && kk < n) ? G[TRANSPOSED ? kk + LD * row : row + LD * kk] : 0.0;
    }
    unsigned kmask = 0;
#pragma unroll
    for (int ks = 0; ks < PL_KS; ++ks)
        if (__ballot(a[ks] != 0.0)) kmask |= 1u << ks;
    return __builtin_amdgcn_readfirstlane(kmask);
}

// one row of a row-compressed matrix (val / col: w entries from eb, zero padded, read from memory) against the column x in LDS, in the row's fixed
// order: a drive's G_l or G_l^T term, a variation's Gv_b or Gv_b^T term.  The chain of fused multiply-adds STARTS from s (s is not a bias added
// behind the sum): a second term handed the first term's result continues that sum entry by entry
__device__ __forceinline__ double pl_row_dot(const double *__restrict__ val, const int *__restrict__ col, long long eb, int w, const double *x, double s = 0.0) {
    for (int e = 0; e < w; ++e) s = __builtin_fma(val[eb + e], x[col[eb + e]], s);
    return s;
}

// nce columns of n doubles, LDS (leading dimension LD) -> memory (contiguous); pairs where the destination allows it
__device__ __forceinline__ void pl_store_cols(double *__restrict__ dst, const double *__restrict__ src, int n, int LD, int nce, int tid, int nth) {
    if (!(n & 1) && !(reinterpret_cast<unsigned long long>(dst) & 15ull)) {
        const int hn = n >> 1;
        for (int e = tid; e < nce * hn; e += nth) {
            const int c = e / hn, i = 2 * (e - c * hn);
            store2(dst + c * n + i, src[i + LD * c], src[i + 1 + LD * c], 0);
        }
    } else {
        for (int e = tid; e < nce * n; e += nth) dst[e] = src[(e % n) + LD * (e / n)];
    }
}
