"""CPU: ic3_env_encode_backward_window_finish_ordered on the host build of the product's own sources — the window form's expansion
with every sum in a fixed order (the partials folded, then one thread per element of dWt): against the dense products in float64,
against the plain finish on the same partials, and unchanged partials afterwards."""
import numpy as np
import pytest

from host_abi_util import check, host_lib, p
from test_host_abi_cpu import ENC_CASES, _make, _play


@pytest.mark.parametrize("kind,cfg", ENC_CASES)
def test_ordered_finish_equals_the_dense_products_and_the_plain_finish(kind, cfg):
    """Every encoder configuration of test_host_abi_cpu.py (PP with vision 0 / 1 / 2 and enemy_comm, TJ easy / medium / hard with
    both vocabularies): dWt = sum_t obs_t^T g_t and dbias = sum_t sum_rows g_t within the plain finish's bar (4e-5 at these sizes),
    the two finishes within rounding of each other, twice the same bits, and the work buffer untouched."""
    env = _make(kind, cfg)
    lib = host_lib()
    H, T = 32, 3
    rng = np.random.default_rng(17)
    n = int(lib.ic3_env_encode_backward_window_work(env._h, H))
    ns = int(lib.ic3_env_encode_backward_window_finish_scratch(env._h, H))
    assert n > 0 and 0 < ns <= n
    assert int(lib.ic3_env_encode_backward_window_finish_scratch(env._h, 24)) == 0     # (no window form: hid_size % 32)
    work = np.full((n,), np.nan, np.float32)
    R = env.E * env.N
    snaps, ring = [], rng.standard_normal((T, R, H)).astype(np.float32)
    want, wantb = 0.0, 0.0
    for k in range(T):
        _play(env, 2 + k, 50 + k)
        snaps.append(env.snapshot())
        obs = env.observe().reshape(-1, env.obs_dim).astype(np.float64)
        want = want + obs.T @ ring[k].astype(np.float64)
        wantb = wantb + ring[k].astype(np.float64).sum(0)
    snaps = np.ascontiguousarray(np.stack(snaps))
    check(lib.ic3_env_encode_backward_window(env._h, p(snaps), snaps.shape[1], T, p(ring), H, R * H, H, p(work), 1, None))
    before = work.copy()
    outs = []
    for _ in range(2):
        dwt = np.full((env.obs_dim, H), np.nan, np.float32)
        db = np.full((H,), np.nan, np.float32)
        scratch = np.full((ns,), np.nan, np.float32)
        check(lib.ic3_env_encode_backward_window_finish_ordered(env._h, H, p(dwt), p(db), p(work), p(scratch), None))
        outs.append((dwt, db))
    dwt, db = outs[0]
    np.testing.assert_allclose(dwt, want, rtol=0, atol=4e-5)
    np.testing.assert_allclose(db, wantb, rtol=0, atol=4e-5)
    assert np.array_equal(outs[1][0], dwt) and np.array_equal(outs[1][1], db)
    assert np.array_equal(work, before, equal_nan=True)
    plain_w = np.full((env.obs_dim, H), np.nan, np.float32)
    plain_b = np.full((H,), np.nan, np.float32)
    check(lib.ic3_env_encode_backward_window_finish(env._h, H, p(plain_w), p(plain_b), p(work), None))
    np.testing.assert_allclose(dwt, plain_w, rtol=0, atol=1e-5)
    np.testing.assert_allclose(db, plain_b, rtol=0, atol=1e-5)
    # without dbias; null arguments
    dwt2 = np.full((env.obs_dim, H), np.nan, np.float32)
    check(lib.ic3_env_encode_backward_window_finish_ordered(env._h, H, p(dwt2), None, p(work), p(scratch), None))
    assert np.array_equal(dwt2, dwt)
    assert lib.ic3_env_encode_backward_window_finish_ordered(env._h, H, p(dwt2), None, p(work), None, None) == -22
    assert lib.ic3_env_encode_backward_window_finish_ordered(None, H, p(dwt2), None, p(work), p(scratch), None) == -22
    env.close()
