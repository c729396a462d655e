"""TEST INFRASTRUCTURE: the bars of tests/test_tanh_walk_gpu.py, case -> quantity -> bar.  Only the two shapes where a workgroup of the
per-step launch owns two tiles have one: there the walk's partial rows (one per tile) are compared as column sums against the
float64 window backward of tests/tanh_window_ref.py.  The bar is 4 x the figure of the PER-STEP call on the same inputs (zeroed
partials; worst |got - ref| / max(1, max |ref|)), because a different but equally long fp32 summation order may land anywhere in
that spread — never above 1e-5.  Measured on the MI355X: profiles/r26/tanh_walk_errors.txt."""
CAP = 1e-5

BARS = {
    'gpu/rnn-h128-pp-n3-E5700-T2-two-tiles-a-workgroup': {
        'dbias_cols': 5.61e-07,                                  # 4 x 1.403e-07
    },
    'gpu/rnn-h64-tj-easy-E6560-T2-collect-two-tiles-a-workgroup': {
        'dbias_cols': 7.06e-07,                                  # 4 x 1.765e-07
    },
}
