// Stand-alone host program of tests/test_cell_prologue_host.py: walks every lattice cell of a list of shapes and checks that
// every index the gradient pass's set-up reads at (csrc/rnnt_lin.h lin_grad_indices -- the set-up fetches all of them
// unconditionally) lies inside its array as csrc/rnnt_common.h make_layout sizes it, and that a clamp never moves the index of an
// edge the cell has.  Runs on the CPU; nothing of it touches a GPU.
//   usage: cell_prologue_host B,T,U [B,T,U ...]      exit status 0 = every index in range
#include "rnnt_lin.h"

#include <stdio.h>
#include <stdlib.h>

#include <vector>

using namespace rnnt;

static long g_checked = 0, g_bad = 0;

static void expect(bool ok, const char *what, int B, int T, int U, int sh, int b, int t, int u) {
    ++g_checked;
    if (ok) return;
    if (g_bad++ < 20) fprintf(stderr, "B%d T%d U%d shift %d: cell (%d, %d, %d): %s\n", B, T, U, sh, b, t, u, what);
}

static void walk(int B, int T, int U) {
    const WsLayout w = make_layout(T, U, B);
    const size_t nLat = (size_t)B * w.Nr * w.Up;    // A, Bt
    const size_t nFrm = (size_t)B * w.NCl * 64;     // EA, EB
    const size_t nLab = (size_t)B * (U - 1);        // labels
    // The arrays themselves, so that the host sanitizers see every access: one byte per element.
    std::vector<unsigned char> lat(nLat, 1), frm(nFrm, 1), lab(nLab ? nLab : 0, 1);
    unsigned long sum = 0;
    for (int sh = 2; sh <= 3; ++sh)  // blocks of four and of eight diagonals
        for (int b = 0; b < B; ++b)
            for (int t = 0; t < T; ++t)
                for (int u = 0; u < U; ++u) {
                    const int n = t + u, l0 = u / w.OG, l1 = (u + 1) / w.OG;
                    const LinIdx x = lin_grad_indices(b, n, u, sh, l0, l1, w.Nr, w.Up, w.NCl, U);
                    const bool in = x.sk < nLat && x.down < nLat && x.diag < nLat && x.e00 < nFrm && x.e10 < nFrm && x.e11 < nFrm &&
                                    (U == 1 || x.lab < nLab);
                    expect(in, "index outside its array", B, T, U, sh, b, t, u);
                    if (!in) continue;
                    sum += lat[x.sk] + lat[x.down] + lat[x.diag] + frm[x.e00] + frm[x.e10] + frm[x.e11] + (U > 1 ? lab[x.lab] : 0);
                    // the clamps are inactive wherever the set-up USES the value
                    const size_t sk = ((size_t)b * w.Nr + n) * w.Up + u, tb = (size_t)b * w.NCl * 64;
                    expect(x.sk == sk && x.e00 == tb + (size_t)(n >> sh) * 64 + l0, "the cell's own indices moved", B, T, U, sh, b, t, u);
                    if (t < T - 1)
                        expect(x.down == sk + w.Up && x.e10 == tb + (size_t)((n + 1) >> sh) * 64 + l0, "blank edge moved", B, T, U, sh, b, t, u);
                    if (u < U - 1)
                        expect(x.diag == sk + w.Up + 1 && x.e11 == tb + (size_t)((n + 1) >> sh) * 64 + l1 && x.lab == (size_t)b * (U - 1) + u,
                               "label edge moved", B, T, U, sh, b, t, u);
                }
    printf("B%d T%d U%d: Nr %d Up %d NCl %d OG %d, checksum %lu\n", B, T, U, w.Nr, w.Up, w.NCl, w.OG, sum);
}

int main(int argc, char **argv) {
    if (argc < 2) {
        fprintf(stderr, "usage: %s B,T,U [B,T,U ...]\n", argv[0]);
        return 2;
    }
    for (int i = 1; i < argc; ++i) {
        int B = 0, T = 0, U = 0;
        if (sscanf(argv[i], "%d,%d,%d", &B, &T, &U) != 3 || B < 1 || T < 1 || U < 1) {
            fprintf(stderr, "bad shape '%s'\n", argv[i]);
            return 2;
        }
        walk(B, T, U);
    }
    printf("%ld checks, %ld failed\n", g_checked, g_bad);
    return g_bad ? 1 : 0;
}
