"""GPU: ic3_policy_forward as a recording inner pass (ops.policy_forward_record: an ic3_policy_record) — one communication pass of a comm_passes > 1 step as a RECORDING inner
pass over a chunk of whole steps — against the float64 pass of tests/bptt_passes_ref.py (gates, inp, h_out, c_out), and against
the plain ic3_policy_forward with inner_pass on copies of the state: the same bits (the record flag does not touch the arithmetic)."""
import numpy as np
import pytest
import torch

import bptt_passes_ref as ref

pytestmark = pytest.mark.gpu

HEADS = [5, 2]

CASES = {
    # tiles are 21 envs = 63 rows: 90 stacked envs = 4 tiles + a ragged one of 6 envs
    'h64-n3-E45-x2': dict(H=64, N=3, E=45, steps=2, pass_index=1),
    'h64-n3-E45-x2-sum': dict(H=64, N=3, E=45, steps=2, pass_index=1, avg=False),
    'h64-n3-E45-x2-comm-zero': dict(H=64, N=3, E=45, steps=2, pass_index=0, comm_zero=True),
    # the steps have different masks, and the second step has no alive mask (ones in the stack)
    'h128-n10-E13-x3': dict(H=128, N=10, E=13, steps=3, pass_index=1, no_alive=1),
    'h256-n32-E5': dict(H=256, N=32, E=5, steps=1, pass_index=1),
}


def make_cache(params, H, dev, passes):
    """The entries of comm.CommNetMLP._fused_cache the policy launches read, from a state_dict-shaped dict of float64 arrays."""
    from ic3net_amd import ops
    t = lambda a: torch.tensor(np.ascontiguousarray(a, np.float32), device=dev)
    w_ih, w_hh = t(params['f_module.weight_ih']), t(params['f_module.weight_hh'])
    fc = ops.policy_step_pack(t(params['C_modules.0.weight']), w_ih, w_hh)
    fc['ps_l_wp3'] = ops.policy_pack_split(w_ih, w_hh)
    fc['b_cat'] = t(params['f_module.bias_ih'] + params['f_module.bias_hh'])
    nh = len(HEADS)
    fc['w_heads'] = t(np.concatenate([params['heads.%d.weight' % k] for k in range(nh)] + [params['value_head.weight']], 0))
    fc['b_heads'] = t(np.concatenate([params['heads.%d.bias' % k] for k in range(nh)] + [params['value_head.bias']], 0))
    for i in range(1, passes):
        fc['ps_c_wp_p%d' % i] = ops.policy_step_pack(t(params['C_modules.%d.weight' % i]), w_ih, w_hh)['ps_c_wp']
        fc['enc_dbias_p%d' % i] = t(params['C_modules.%d.bias' % i] - params['C_modules.0.bias'])
    return fc


@pytest.mark.parametrize("name", list(CASES))
def test_forward_record_against_float64_and_the_inner_pass(name):
    from ic3net_amd import ops
    from test_host_policy_step_cpu import make_params
    cfg = CASES[name]
    H, N, E, S, pi = cfg['H'], cfg['N'], cfg['E'], cfg['steps'], cfg['pass_index']
    avg, comm_zero = cfg.get('avg', True), cfg.get('comm_zero', False)
    dev = torch.device('cuda:0')
    Et, R = S * E, S * E * N
    rng = np.random.default_rng(sum(map(ord, name)))
    params = make_params(12, H, HEADS, seed=H + N, comm_passes=2)
    fc = make_cache(params, H, dev, 2)
    f32 = lambda a: np.ascontiguousarray(a, np.float32)
    x = f32(rng.standard_normal((R, H)))                          # encoder(obs) + encoder.bias
    enc = f32(x + f32(params['C_modules.0.bias']))                # ... + C_0.bias: the encoder ring's rows
    h0, c0 = f32(np.tanh(rng.standard_normal((R, H)))), f32(rng.standard_normal((R, H)))
    alive = np.ascontiguousarray(rng.random((S, E, N)) < 0.8, np.int32)
    alive[0, 0] = 0                                               # an env with nobody alive, one with a single agent alive
    alive[0, 1] = 0
    alive[0, 1, N // 2] = 1
    if 'no_alive' in cfg:
        alive[cfg['no_alive']] = 1
    gate = np.ascontiguousarray(rng.random((S, E, N)) < 0.6, np.int32)
    up = lambda a: torch.from_numpy(a).to(dev)
    add = fc['enc_dbias_p1'] if pi else None
    xw = ops.record_xh_width(H)

    def launch():
        h_in, c_in = up(h0), up(c0)
        out = dict(h=torch.full((R, H), float('nan'), device=dev), c=torch.full((R, H), float('nan'), device=dev),
                   gates=torch.full((R, 4 * H), float('nan'), device=dev), inp=torch.full((R, xw), float('nan'), device=dev))
        ops.policy_forward_record(fc, H, HEADS, avg, comm_zero, up(enc), Et, N, h_in, c_in, out['h'], out['c'], up(alive), up(gate),
                                  out['gates'], out['inp'], pass_index=pi, enc_add=add)
        torch.cuda.synchronize()
        assert torch.equal(h_in.cpu(), torch.from_numpy(h0)) and torch.equal(c_in.cpu(), torch.from_numpy(c0))   # the inputs keep their bits
        return out

    got = launch()
    again = launch()
    for k in got:
        assert torch.equal(got[k].view(torch.int32), again[k].view(torch.int32)), k       # (bit patterns: NaN-filled tails compare equal)
    # ic3_policy_forward as an inner pass, in place on copies, on enc + (C_i.bias - C_0.bias) added by the caller
    h, c = up(h0), up(c0)
    enc_i = up(enc) if add is None else torch.add(up(enc), add)
    ops.policy_forward(fc, H, HEADS, avg, comm_zero, enc_i, Et, N, h, c, up(alive), up(gate), pass_index=pi, inner=True)
    torch.cuda.synchronize()
    assert torch.equal(got['h'], h) and torch.equal(got['c'], c)
    if H != 256:
        assert bool(torch.isnan(got['inp'][:, H:]).all())        # the h half of the [inp | h] rows is not touched
    # float64: the pass on E x steps envs (the masks differ per step; the mix never crosses an env)
    a64, inp64, h64, c64 = ref.pass_forward(x, h0, c0, params['C_modules.%d.weight' % pi], params['C_modules.%d.bias' % pi],
                                            params['f_module.weight_ih'], params['f_module.weight_hh'],
                                            params['f_module.bias_ih'] + params['f_module.bias_hh'], Et, N, alive.reshape(Et, N),
                                            gate.reshape(Et, N), avg, comm_zero)
    num = lambda v: v.double().cpu().numpy()
    ref.check('gpu/fwd-' + name, dict(fwd_gates=ref.rel_err(num(got['gates']), a64), fwd_inp=ref.rel_err(num(got['inp'][:, :H]), inp64),
                                      fwd_h=ref.rel_err(num(got['h']), h64), fwd_c=ref.rel_err(num(got['c']), c64)))


def test_forward_record_needs_the_split_planes():
    """Without lstm_wp3 the call refuses (NotImplementedError) and writes nothing."""
    from ic3net_amd import ops
    from test_host_policy_step_cpu import make_params
    dev = torch.device('cuda:0')
    H, N, E = 64, 3, 4
    fc = make_cache(make_params(12, H, HEADS, seed=1, comm_passes=2), H, dev, 2)
    del fc['ps_l_wp3']
    z = lambda w: torch.zeros((E * N, w), device=dev)
    g = torch.full((E * N, 4 * H), float('nan'), device=dev)
    with pytest.raises(NotImplementedError, match="gate_split"):
        ops.policy_forward_record(fc, H, HEADS, True, False, z(H), E, N, z(H), z(H), z(H), z(H), None, None, g, z(2 * H))
    torch.cuda.synchronize()
    assert bool(torch.isnan(g).all())
