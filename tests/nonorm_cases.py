"""Op rows of the depthwise + pointwise family WITHOUT a norm layer (target_ops.dwpw), shared by tests/test_nonorm_cpu.py (the
rows are well conditioned) and tests/test_gpu_target_nonorm.py (the kernels against fp64): the edge rows of
tests/target_edge_cases.py through its own generators -- gamma and beta ignored -- plus two rows BatchNorm cannot have or does
not pin."""
import target_edge_cases as E

# N, C_in, C_out, H, W, ks, stride, pad, dil, gain
DWPW_ROWS = E.DWPW_ROWS + [
    (1, 12, 20, 3, 3, 3, 1, 0, 1, 1.0),           # ONE output pixel (F.batch_norm refuses P = 1 in training mode)
]
# N, C_in, C_out, H, W, stride
PW_ROWS = E.PW_ROWS + [
    (33, 8, 12, 1, 2, 1),                         # P = 66: one full tile plus a 2-pixel tile; a tile spans 32 samples
]


def dwpw_case(row):
    """(x, w_dw, w_pw, upstream gradient, (ks, stride, pad, dil)) of a DWPW row, fp32 on the CPU."""
    x, w_dw, w_pw, _, _, up = E.dwpw_inputs(row)
    return x, w_dw, w_pw, up, tuple(row[5:9])


def pw_case(row):
    """(x, w_pw, upstream gradient, stride) of a PW row."""
    x, w_pw, _, _, up = E.pw_inputs(row)
    return x, w_pw, up, row[5]
