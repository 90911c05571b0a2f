// Stand-alone driver of csrc/conv_forms.h (no HIP, no GPU): prints the two tables and the picks over a sweep of queries, for
// tests/test_conv_forms_cpu.py to hold against tests/forms_model.py.  Built with -fsanitize=address,undefined.
//
// Output:
//   T i kernel ct rows ring full pl prod npl epi hook       one line per row of kTrunkForms
//   R i <the 12 fields of trunk_form_record(row i)>
//   L i form ct epi up waves np ring hpo occ f8 ph full      one line per row of kTailForms
//   G N H W m <codes>      trunk picks of one geometry (m: index into kMos); one code per (small8, f16_full, ct, epi, fp8, nstage,
//                          hook), nested in this order, the last fastest
//   C form <codes>         launch_conv picks of one ConvForm value; codes over (H, W, m, f16_full, slope, src_lo)
//   P py f8 <codes>        launch_conv_phase picks; codes over (H, W, m, f16_full)
// A code is 'A' + row, '-' for kFormNotSupported, '!' for kFormInvalid.
#include <stdio.h>
#include <stdlib.h>

#include <string>

#include "conv_forms.h"

using namespace s2sr;

static const int kN[] = {1, 2, 3, 6, 9, 16, 20, 32};
static const int kHW[] = {8, 16, 20, 32, 37, 53, 64, 96, 100, 192, 256, 276, 300, 320, 330, 553, 1024};
static const int kMos[][4] = {{0, 0, 0, 0}, {277, 276, 277, 276}, {21, 20, 21, 20}, {101, 100, 101, 100}};
static const int kStages[] = {2, 4, 6};

static char code(int r, int rows) {
    if (r == kFormNotSupported) return '-';
    if (r == kFormInvalid) return '!';
    if (r < 0 || r >= rows) { fprintf(stderr, "pick answered %d\n", r); abort(); }
    return (char)('A' + r);
}

int main() {
    for (int i = 0; i < TF_COUNT; ++i) {
        const TrunkForm& f = kTrunkForms[i];
        printf("T %d %d %d %d %d %d %d %d %d %d %d\n", i, f.kernel, f.ct, f.rows, f.ring, f.full, f.pl, f.prod, f.npl, f.epi, f.hook);
        const s2sr_debug_trunk_form r = trunk_form_record(f);
        printf("R %d %d %d %d %d %d %d %d %d %d %d %d %d\n", i, r.kernel, r.ct, r.rows, r.ring, r.full, r.pl, r.prod, r.wgl, r.loe, r.wv, r.npl, r.epi);
    }
    for (int i = 0; i < kTailFormCount; ++i) {
        const TailForm& f = kTailForms[i];
        printf("L %d %d %d %d %d %d %d %d %d %d %d %d %d\n", i, f.form, f.ct, f.epi, (int)f.up, f.waves, f.np, f.ring, f.hpo, f.occ, (int)f.f8, f.ph, (int)f.full);
    }
    std::string line;
    for (int N : kN)
        for (int H : kHW)
            for (int W : kHW)
                for (int m = 0; m < 4; ++m) {
                    line.clear();
                    for (int small8 = 0; small8 < 2; ++small8)
                        for (int full = 0; full < 2; ++full)
                            for (int ct = 1; ct <= 2; ++ct)
                                for (int epi = 0; epi < 4; ++epi)
                                    for (int fp8 = 0; fp8 < 2; ++fp8)
                                        for (int nstage : kStages)
                                            for (int hook = 0; hook <= 12; ++hook) {
                                                TrunkQuery q{};
                                                q.N = N; q.H = H; q.W = W;
                                                q.mos_py = kMos[m][0]; q.mos_ry = kMos[m][1]; q.mos_px = kMos[m][2]; q.mos_rx = kMos[m][3];
                                                q.ct = ct; q.epi = epi; q.fp8 = fp8 != 0; q.nstage = nstage;
                                                q.sw.small8 = small8 != 0; q.sw.f16_full = full != 0; q.hook = hook;
                                                line.push_back(code(pick_trunk_form(q), TF_COUNT));
                                            }
                    printf("G %d %d %d %d %s\n", N, H, W, m, line.c_str());
                }
    for (int form = -1; form <= CF_DEBUG2_UP + 1; ++form) {
        line.clear();
        for (int H : kHW)
            for (int W : kHW)
                for (int m = 0; m < 4; ++m)
                    for (int full = 0; full < 2; ++full)
                        for (int slope = 0; slope < 2; ++slope)
                            for (int lo = 0; lo < 2; ++lo) {
                                TailQuery q{};
                                q.form = form; q.H = H; q.W = W; q.mos_py = kMos[m][0];
                                q.slope = slope != 0; q.src_lo = lo != 0; q.sw.f16_full = full != 0;
                                line.push_back(code(pick_tail_form(q), kTailFormCount));
                            }
        printf("C %d %s\n", form, line.c_str());
    }
    for (int py = -1; py <= 2; ++py)
        for (int f8 = 0; f8 < 2; ++f8) {
            line.clear();
            for (int H : kHW)
                for (int W : kHW)
                    for (int m = 0; m < 4; ++m)
                        for (int full = 0; full < 2; ++full) {
                            FormSwitches sw;
                            sw.f16_full = full != 0;
                            line.push_back(code(pick_phase_form(py, f8 != 0, H, W, kMos[m][0], sw), kTailFormCount));
                        }
            printf("P %d %d %s\n", py, f8, line.c_str());
        }
    printf("ok\n");
    return 0;
}
