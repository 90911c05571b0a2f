"""The trunk kernel forms the shipped picks reach with the default switches and no hook number: asserted against csrc/conv_forms.h
without a GPU (test_conv_forms_cpu.py), and every one of them must be seen in the form records of a GPU run
(test_gpu_trunk_insitu.py)."""
# Every conv_trunk instantiation the shipped dispatcher picks with the default switches, as (kernel, ct, rows, ring, full, pl,
# prod, npl, epi) -- epi 0: conv1-4, 1: conv5 of rdb1 / rdb2, 2: conv5 of rdb3.  test_conv_forms_cpu.py fails when the
# table of csrc/conv_forms.h and this list disagree.
PRODUCTION_FORMS = {
    (1, 1, 8, 3, 1, 2, 0, 0, 0), (1, 1, 8, 3, 3, 2, 0, 0, 0), (1, 1, 8, 7, 0, 1, 0, 0, 0),          # conv1-4, n32 < 96
    (1, 1, 16, 5, 1, 1, 0, 0, 0), (1, 1, 16, 5, 3, 1, 0, 0, 0), (1, 1, 16, 5, 0, 1, 0, 0, 0),       # conv1-4, 96 <= n32 < 192
    (1, 1, 32, 3, 1, 1, 0, 0, 0), (1, 1, 32, 3, 3, 1, 0, 0, 0), (1, 1, 32, 3, 2, 1, 0, 0, 0),       # conv1-4, n32 >= 192
    (1, 1, 32, 3, 0, 1, 0, 0, 0),
    (1, 2, 8, 2, 0, 2, 0, 0, 1), (1, 2, 8, 2, 0, 2, 0, 0, 2),                                        # conv5, n16 < 192
    (1, 2, 16, 4, 0, 1, 0, 0, 1), (1, 2, 16, 4, 0, 1, 0, 0, 2),                                      # conv5, n16 >= 192
    (2, 1, 16, 6, 0, 2, 1, 4, 0), (2, 1, 16, 6, 0, 2, 1, 0, 0),                                      # fp8 conv1-3, conv4
    (2, 2, 16, 4, 0, 2, 0, 0, 1), (2, 2, 16, 4, 0, 2, 0, 0, 2),                                      # fp8 conv5
}
