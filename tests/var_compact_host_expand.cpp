// Stand-alone check of the host expanders of a variational context (pcl_host_expand.hpp: expand_interval_var, expand_interval_var_exp):
// both halves, at every store width this host has, against a plain loop, with guard words around the output.  Built and run by
// tests/test_var_compact_cpu.py; also meant to be built with -fsanitize=address,undefined by hand.  Exit status 0: every check passed.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "pcl_host_expand.hpp"

static int fails = 0;

static void check(const char *what, int n, int C, int v, int m, int width, int expo) {
    const long long nn = (long long)n * n, xd = (long long)(1 + v) * n * C, tail = xd * (m + 1);
    const int ntile = expo ? 1 + v : 2 + 2 * v, nseg = expo ? 1 + 2 * v : 2 + 4 * v;
    const long long cper = ntile * nn + tail, fper = nseg * C * nn + (expo ? xd : 0) + tail;
    std::vector<double> comp((size_t)cper);
    for (long long e = 0; e < cper; ++e) comp[(size_t)e] = 1000.0 + (double)e * 0.5;  // every compact value distinct, none of them 1.0
    // the plain loop
    std::vector<double> want((size_t)fper);
    long long o = 0;
    for (int s = 0; s < nseg; ++s) {
        int t;
        if (expo)
            t = (s == 0 || (s & 1)) ? 0 : s / 2;
        else if (s < 2)
            t = s;
        else
            t = ((s - 2) % 4 < 2) ? (s - 2) % 4 : 2 + 2 * ((s - 2) / 4) + ((s - 2) % 4 - 2);
        for (int c = 0; c < C; ++c)
            for (long long e = 0; e < nn; ++e) want[(size_t)o++] = comp[(size_t)(t * nn + e)];
    }
    if (expo)
        for (long long e = 0; e < xd; ++e) want[(size_t)o++] = 1.0;
    for (long long e = 0; e < tail; ++e) want[(size_t)o++] = comp[(size_t)(ntile * nn + e)];
    if (o != fper) {
        printf("FAIL %s: the plain loop wrote %lld of %lld values\n", what, o, fper);
        ++fails;
        return;
    }
    int chosen = 0;
    const pcl_host::stream_copy_fn copy = pcl_host::pick_stream_copy(width, &chosen);
    const double guard = -7.25;
    const int G = 16;
    // the two halves in both orders, and each half alone (it must write its part only, and the two parts must be disjoint and complete)
    for (int order = 0; order < 2; ++order) {
        std::vector<double> buf((size_t)fper + 2 * G, guard);
        std::vector<int> hits((size_t)fper, 0);
        for (int hh = 0; hh < 2; ++hh) {
            const int half = order ? 1 - hh : hh;
            std::vector<double> one((size_t)fper + 2 * G, guard);
            if (expo)
                pcl_host::expand_interval_var_exp(one.data() + G, comp.data(), C, nn, v, xd, tail, half, copy);
            else
                pcl_host::expand_interval_var(one.data() + G, comp.data(), C, nn, v, tail, half, copy);
            for (int g = 0; g < G; ++g)
                if (one[(size_t)g] != guard || one[(size_t)(G + fper + g)] != guard) {
                    printf("FAIL %s width %d half %d: a guard word was overwritten\n", what, chosen, half);
                    ++fails;
                }
            for (long long e = 0; e < fper; ++e)
                if (one[(size_t)(G + e)] != guard) {
                    ++hits[(size_t)e];
                    buf[(size_t)(G + e)] = one[(size_t)(G + e)];
                }
        }
        long long bad = 0, multi = 0;
        for (long long e = 0; e < fper; ++e) {
            if (memcmp(&buf[(size_t)(G + e)], &want[(size_t)e], sizeof(double)) != 0) ++bad;
            if (hits[(size_t)e] != 1) ++multi;
        }
        if (bad || multi) {
            printf("FAIL %s width %d: %lld wrong values, %lld values not written exactly once by the two halves\n", what, chosen, bad, multi);
            ++fails;
        }
    }
    printf("ok   %s (n=%d C=%d v=%d m=%d) store width %d: %lld -> %lld values\n", what, n, C, v, m, chosen, cper, fper);
}

int main() {
    static const int shapes[4][4] = {{4, 1, 1, 2}, {8, 4, 2, 4}, {34, 17, 1, 3}, {54, 27, 2, 6}};  // (n, C, v, m)
    int widest = 0;
    (void)pcl_host::pick_stream_copy(0, &widest);
    int ran = 0;
    for (int width = 16; width <= widest; width *= 2)
        for (const auto &s : shapes) {
            check("expand_interval_var    ", s[0], s[1], s[2], s[3], width, 0);
            check("expand_interval_var_exp", s[0], s[1], s[2], s[3], width, 1);
            ran += 2;
        }
    printf("%d checks at store widths 16 .. %d bytes, %d failures\n", ran, widest, fails);
    return fails ? 1 : 0;
}
