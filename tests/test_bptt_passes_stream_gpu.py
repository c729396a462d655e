"""GPU: ic3_bptt_backward on an ic3_bptt_passes descriptor with the collection-mode row factors, through ops.bptt_passes_backward
(row_keep / keep_before), against the float64 collection-mode window backward of tests/bptt_passes_stream_ref.py — the cases, what
the caller does around the call and the assertions of tests/bptt_passes_stream_cases.py, shared with the host-build test; this file
is the device backend and the refusal."""
import numpy as np
import pytest
import torch

import bptt_passes_stream_cases as cases

pytestmark = pytest.mark.gpu


def make_env(spec):
    from test_env_parity_gpu import make_pp, make_tj
    kind, N, dim, E = spec
    if kind == 'pp':
        return make_pp(N, dim, 1, 'mixed', E, seed=3)
    return make_tj(N, dim, 1, 'easy', E, seed=3, add_rate_min=0.5, add_rate_max=0.5)


class Device(object):
    """A case's arrays on the device and the buffers a run writes"""

    def __init__(self, env, case, snaps):
        from ic3net_amd import ops
        dev = env.device
        P, T, R, H = case.P, case.T, case.R, case.H
        self.up = up = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        w = case.w
        self.dgates, self.hs, self.cs = up(w['gates']), up(case.hs_in), up(case.cs_in)
        self.dh, self.dc, self.dhead, self.snaps = up(case.dh_in), up(w['dc']), up(w['dhead']), snaps
        self.dxh = torch.full((P, T, R, 2 * H), float('nan'), device=dev)
        self.bias = up(case.bias0)
        self.dcw0 = None if case.comm_zero else torch.randn((P, ops.comm_backward_partials(case.E, case.N), H, H),
                                                            generator=torch.Generator().manual_seed(98))
        self.dcw = None if case.comm_zero else self.dcw0.to(dev)
        self.wb3 = ops.policy_pack_split_bwd(up(w['w_ih']), up(w['w_hh']))
        self.w_heads = up(w['w_heads'])
        cws = {id(a): up(a) for a in w['c_weights']}
        self.cws = None if case.comm_zero else [cws[id(a)] for a in w['c_weights']]
        self.alive = None if case.alive is None else [up(m) for m in case.alive]
        self.gate = None if case.gate is None else [up(m) for m in case.gate]
        self.keep = up(case.keep_rows)
        self.env, self.case = env, case

    def call(self, t0, t1, first, factors=True, gap=0):
        from ic3net_amd import ops
        case, P = self.case, self.case.P
        sl = lambda x: [x[i, t0:t1] for i in range(P)]
        ops.bptt_passes_backward(self.env, t1 - t0, case.E, case.N, case.H, sl(self.dgates), sl(self.hs), sl(self.cs), self.dhead[t0:t1],
                                 self.snaps[t0:t1], None if self.alive is None else self.alive[t0:t1],
                                 None if self.gate is None else self.gate[t0:t1], self.wb3, self.w_heads, self.cws, self.dh, self.dc,
                                 sl(self.dxh), [self.bias[i] for i in range(P)],
                                 None if case.comm_zero else [self.dcw[i] for i in range(P)], mode_avg=case.avg, comm_zero=case.comm_zero,
                                 detach_gap=gap, t_first=t0, enc_first=first, row_keep=self.keep[t0:t1] if factors else None,
                                 keep_before=self.keep[t0 - 1] if factors and t0 > 0 else None)


def run(case, most):
    from ic3net_amd import ops
    from test_bptt_passes_gpu import _snapshots
    env = make_env(case.cfg['env'])
    assert (env.nenvs, env.nagents_env) == (case.E, case.N) and ops.bptt_passes_backward_supported(env, case.H, case.P)
    snaps, obs = _snapshots(env, case.T)
    d = Device(env, case, snaps)
    first = True
    for t0, t1 in cases.chunks(case.T, most or case.T):
        d.call(t0, t1, first)
        first = False
    dwt, db = env.encode_backward_window_finish(case.H)
    dW = d.up(case.dW0)
    Q = case.P * case.T * case.R
    ops.lstm_weight_grad(d.up(case.w['inp']).reshape(Q, case.H), d.hs.reshape(Q, case.H), d.dgates, dW)
    torch.cuda.synchronize()
    num = lambda v: None if v is None else v.cpu().numpy()
    return dict(dgates=num(d.dgates), dxh=num(d.dxh), dh=num(d.dh), dc=num(d.dc), bias=num(d.bias), dcw=num(d.dcw), dcw0=num(d.dcw0),
                enc_dwt=num(dwt), enc_db=num(db), dW=num(dW)), obs


@pytest.mark.parametrize("name", list(cases.CASES))
def test_passes_backward_with_row_factors_against_float64(name):
    """Every buffer the call writes or adds to, for the window in one call and in chunks of 2 slots, each against the float64
    reference of the whole window at its bar (what tests/test_host_bptt_passes_stream_cpu.py asserts on the host build)."""
    cases.run_and_check('gpu', name, run)


def test_detach_gap_with_row_factors_is_refused_and_null_factors_change_nothing():
    """detach_gap > 0 with row factors: ValueError before any launch, the records keep their bits.  Factors of 1.0 everywhere against
    no factors at all: the same bits; the case's real factors: other bits."""
    from test_bptt_passes_gpu import _snapshots
    case = cases.Case('h64-tj-n5-E13-T4-P2-comm-zero-independent')
    env = make_env(case.cfg['env'])
    snaps, _ = _snapshots(env, case.T)
    d = Device(env, case, snaps)
    with pytest.raises(ValueError, match="detach_gap > 0 with row_keep"):
        d.call(0, case.T, True, gap=2)
    torch.cuda.synchronize()
    assert torch.equal(d.dgates.cpu(), torch.from_numpy(case.w['gates'])) and torch.equal(d.dc.cpu(), torch.from_numpy(case.w['dc']))
    assert torch.equal(d.bias.cpu(), torch.from_numpy(case.bias0)) and bool(torch.isnan(d.dxh).all())
    outs = []
    for mode in ('null', 'ones', 'real'):
        d = Device(env, case, snaps)
        if mode == 'ones':
            d.keep = torch.ones_like(d.keep)
        d.call(0, case.T, True, factors=mode != 'null')
        torch.cuda.synchronize()
        outs.append(d)
    for k in ('dgates', 'dxh', 'dh', 'dc', 'bias'):
        assert torch.equal(getattr(outs[0], k), getattr(outs[1], k)), k
    assert not torch.equal(outs[0].dgates, outs[2].dgates) and not torch.equal(outs[0].dh, outs[2].dh)
