"""Host build: the launch-chain kernels of csrc/policy_ops.hip (ic3_lstm_cell, ic3_lstm_cell_backward, ic3_policy_heads,
ic3_lstm_cell_heads, ic3_comm_masked_mean[_add], ic3_sample_actions) against the float64 references of tests/policy_ops_ref.py —
the twin of tests/test_policy_ops_gpu.py: the same cases and assertions (policy_ops_ref.run_*), bar keys with the host/ prefix."""
import ctypes as C

import numpy as np
import pytest

import policy_ops_ref as ref
from host_abi_util import HostEnv, check, host_lib, p

PREFIX = 'host/'
NAN = np.nan


def at(a, col):
    """Pointer of column `col` of the first row of a float32 array."""
    return C.c_void_p(a.ctypes.data + 4 * col)


def i32(a):
    return None if a is None else np.ascontiguousarray(a, np.int32)


class HostBackend(object):
    def __init__(self):
        self.lib = host_lib()

    def cell_backward(self, gates, c_prev, dh, dc, alias, parts):
        R, H = c_prev.shape
        dg = np.full((R, 4 * H), NAN, np.float32)
        dcp = dc.copy() if alias else np.full((R, H), NAN, np.float32)
        pr = np.full((ref.MAX_PARTIALS, 4 * H), NAN, np.float32) if parts else None
        n = check(self.lib.ic3_lstm_cell_backward(p(gates), p(c_prev), p(dh), p(dcp if alias else dc), p(dg), p(dcp), p(pr), R, H,
                                                  None))
        return n, dg, dcp, pr

    def cell_forward(self, gates, c, H):
        R = c.shape[0]
        c1 = c.copy()
        xh = np.full((R, 2 * H + ref.PAD), NAN, np.float32)
        check(self.lib.ic3_lstm_cell(p(gates), p(c1), at(xh, H + ref.PAD), xh.shape[1], R, H, None))
        return c1, xh

    def heads(self, xh, H, W, b, sizes):
        R = xh.shape[0]
        out = np.full((R, W.shape[0]), NAN, np.float32)
        check(self.lib.ic3_policy_heads(at(xh, H + ref.PAD), xh.shape[1], p(W), p(b), p(i32(sizes)), len(sizes), p(out), R, H, None))
        return out

    def cell_heads(self, gates, c, H, W, b, sizes, env):
        R = c.shape[0]
        c1 = c.copy()
        xh = np.full((R, 2 * H + ref.PAD), NAN, np.float32)
        out = np.full((R, W.shape[0]), NAN, np.float32)
        act = np.full((len(sizes), env.E, env.N), -1, np.int32) if env is not None else None
        check(self.lib.ic3_lstm_cell_heads(p(gates), p(c1), at(xh, H + ref.PAD), xh.shape[1], R, H, p(W), p(b), p(i32(sizes)),
                                           len(sizes), p(out), env._h if env is not None else None, p(act), None))
        return c1, xh, out, act

    def comm(self, h, H, alive, gate, avg, mask_self, addend, add_col0, row_scale):
        E, N, ldh = h.shape
        out = np.full((E, N, H), NAN, np.float32)
        if addend is None:
            check(self.lib.ic3_comm_masked_mean(p(h), ldh, p(i32(alive)), p(i32(gate)), p(out), E, N, H, int(avg), int(mask_self),
                                                None))
        else:
            check(self.lib.ic3_comm_masked_mean_add(p(h), ldh, p(i32(alive)), p(i32(gate)), at(addend, add_col0), addend.shape[2],
                                                    p(row_scale), p(out), E, N, H, int(avg), int(mask_self), None))
        return out

    def sample(self, wide, col0, A, head, seed, offset, episode, t):
        E, N, OT = wide.shape
        act = np.full((E, N), -1, np.int32)
        chosen = np.full((E, N), NAN, np.float32)
        check(self.lib.ic3_sample_actions(at(wide, col0), OT, A, head, seed, offset, episode, t, p(act), p(chosen), E, N, None))
        return act, chosen

    def sample_env(self, env, wide, col0, A, head):
        act = np.full((env.E, env.N), -1, np.int32)
        check(self.lib.ic3_env_sample_actions(env._h, at(wide, col0), wide.shape[2], A, head, p(act), None, None))
        return act

    def make_env(self, E, N):
        env = HostEnv.pp(N, 8, 1, "mixed", E, seed=9, offset=4)
        env.reset()
        rng = np.random.default_rng(E + N)
        for _ in range(3):                                  # move the (episode, t) counters of the draws off zero
            env.step(rng.integers(0, 5, (E, N)), with_obs=False)
        return env

    def env_counters(self, env):
        st = env.get_state()
        return 9, 4, st['episode'].reshape(-1), st['t'].reshape(-1)

    def refusal(self, which):
        H, sizes = ref.refusal_args(which)
        R, OT = 3, sum(sizes) + 1
        z = lambda *s: np.zeros(s, np.float32)
        if which.startswith('cell_backward'):
            check(self.lib.ic3_lstm_cell_backward(p(z(R, 4 * H)), p(z(R, H)), p(z(R, H)), None, p(z(R, 4 * H)), p(z(R, H)), None, R, H,
                                                  None))
        elif which.startswith('cell_heads'):
            self.cell_heads(z(R, 4 * H), z(R, H), H, z(OT, H), z(OT), sizes, None)
        else:
            self.heads(z(R, 2 * H + ref.PAD), H, z(OT, H), z(OT), sizes)


@pytest.fixture(scope="module")
def be():
    return HostBackend()


@pytest.mark.parametrize("case", ref.cell_backward_cases(), ids=ref.cell_backward_id)
def test_cell_backward_against_float64(be, case):
    ref.run_cell_backward(be, PREFIX, *case)


@pytest.mark.parametrize("H", ref.CELL_FWD_H)
def test_cell_forward_against_float64(be, H):
    ref.run_cell_forward(be, PREFIX, H)


@pytest.mark.parametrize("H", ref.HEADS_H)
def test_policy_heads_against_float64(be, H):
    ref.run_heads(be, PREFIX, H)


@pytest.mark.parametrize("H", ref.FUSED_H)
def test_fused_cell_heads_against_float64_and_the_oracle_draw(be, H):
    ref.run_fused(be, PREFIX, H)


@pytest.mark.parametrize("case", ref.comm_cases(), ids=ref.comm_id)
def test_comm_block_against_the_literal_form(be, case):
    ref.run_comm(be, PREFIX, case)


@pytest.mark.parametrize("E,N", ref.SAMPLE_EN)
@pytest.mark.parametrize("A", ref.SAMPLE_A)
def test_sample_actions_against_the_oracle_draw(be, A, E, N):
    ref.run_sample(be, A, E, N)


def test_sample_actions_never_draws_a_zero_probability(be):
    ref.run_sample(be, 5, 51, 5, zero_prob=True)


@pytest.mark.parametrize("which", sorted(ref.REFUSALS))
def test_refusals_are_argument_checks(be, which):
    ref.run_refusal(be, which)
