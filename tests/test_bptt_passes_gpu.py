"""GPU: ic3_bptt_backward on an ic3_bptt_passes descriptor (ops.bptt_passes_backward) — the backward through a window of a comm_passes > 1 recurrent policy as
ONE host call — against the float64 multi-pass window backward of tests/bptt_passes_ref.py on synthetic records over real env
snapshots: which pass gets the heads' share, which one a detach point cuts, the per-pass records, rings and partials, shared C
weights, the encoder's window stage once per pass.  Every case is launched a second time on fresh copies: bit-identical.  The
chunked case runs the whole driver (bptt._backward_window_multipass: encoder ring, recording forward, backward, weight gradient per
chunk) with two steps per chunk against the unchunked run."""
import numpy as np
import pytest
import torch

import bptt_passes_ref as ref

pytestmark = pytest.mark.gpu

OT = 6


def _pp(N, dim, vision, E):
    from test_env_parity_gpu import make_pp
    return make_pp(N, dim, vision, 'mixed', E, seed=3)


def _tj(N, dim, difficulty, E):
    from test_env_parity_gpu import make_tj
    return make_tj(N, dim, 1, difficulty, E, seed=3, add_rate_min=0.5, add_rate_max=0.5)


CASES = {
    'h128-pp-n10-dim20-E131-T3-P2-gap2': dict(env=lambda: _pp(10, 20, 1, 131), H=128, T=3, P=2, gap=2),
    'h64-pp-n3-E200-T4-P3-share-sum': dict(env=lambda: _pp(3, 6, 1, 200), H=64, T=4, P=3, share=True, avg=False, alive='first_null'),
    'h64-tj-n5-E130-T3-P2-comm-zero': dict(env=lambda: _tj(5, 6, 'easy', 130), H=64, T=3, P=2, comm_zero=True, alive='all'),
    # 32 agents need 33 cells: dim 6 is the smallest grid ic3_pp_create takes
    'h256-pp-n32-dim6-E130-T2-P2': dict(env=lambda: _pp(32, 6, 1, 130), H=256, T=2, P=2),
}


def _snapshots(env, T, seed=7):
    """T snapshots two random steps apart and the dense observation rows of each, float64."""
    rng = np.random.default_rng(seed)
    E, N = env.nenvs, env.nagents_env
    env.reset()
    snaps = torch.empty((T, env.dims.state_words), dtype=torch.int32, device=env.device)
    obs = []
    for t in range(T):
        for _ in range(2):
            env.step(rng.integers(0, env.dims.naction, (E, N)), observe=False)
        env.snapshot(out=snaps[t])
        obs.append(env.observe().reshape(E * N, env.obs_dim).double().cpu().numpy())
    return snaps, obs


def _launch(env, w, cfg, snaps):
    """One ops.bptt_passes_backward on fresh device copies; returns the buffers it wrote (NaN-filled / pre-filled with known values)."""
    from ic3net_amd import ops
    dev = env.device
    T, E, N, H, P = w['T'], w['E'], w['N'], w['H'], w['P']
    R = E * N
    up = lambda a: None if a is None else torch.from_numpy(a).to(dev)
    ups = lambda ms: None if ms is None else [up(m) for m in ms]
    gates, dh, dc = up(w['gates']), up(w['dh']), up(w['dc'])
    hs, cs = up(w['hs']), up(w['cs'])
    dxh = torch.full((P, T, R, 2 * H), float('nan'), device=dev)
    g = torch.Generator().manual_seed(99)
    bias0 = torch.randn((P, (R + 63) // 64, 4 * H), generator=g)
    dcw0 = torch.randn((P, ops.comm_backward_partials(E, N), H, H), generator=g)
    bias, dcw = bias0.to(dev), dcw0.to(dev)
    comm_zero = cfg.get('comm_zero', False)
    wb3 = ops.policy_pack_split_bwd(up(w['w_ih']), up(w['w_hh']))
    cws = {id(a): up(a) for a in w['c_weights']}                 # (shared: the same tensor P times)
    out = dict(gates=gates, dh=dh, dc=dc, dxh=dxh, bias=bias, dcw=dcw, bias0=bias0, dcw0=dcw0)
    ops.bptt_passes_backward(env, T, E, N, H, [gates[i] for i in range(P)], [hs[i] for i in range(P)], [cs[i] for i in range(P)],
                             up(w['dhead']), snaps, ups(w['alive']), ups(w['gate']), wb3, up(w['w_heads']),
                             None if comm_zero else [cws[id(a)] for a in w['c_weights']], dh, dc, [dxh[i] for i in range(P)],
                             [bias[i] for i in range(P)], None if comm_zero else [dcw[i] for i in range(P)],
                             mode_avg=cfg.get('avg', True), comm_zero=comm_zero, detach_gap=cfg.get('gap', 0))
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("name", list(CASES))
def test_passes_backward_against_float64(name):
    """dgates of every (t, i), the dxh rings, dh / dc leaving the window, every row of each pass's bias partials, each pass's dcw sum,
    the C_i.bias gradient read off the bias partials, the encoder's dWt / db through the window finish, dW of ops.lstm_weight_grad over
    the P x T x R rows — against float64, each at its bar; then the same call on fresh copies: dgates, dh, dc and both partial buffers
    the same bits."""
    from ic3net_amd import ops
    cfg = CASES[name]
    env = cfg['env']()
    dev = env.device
    T, H, P = cfg['T'], cfg['H'], cfg['P']
    E, N = env.nenvs, env.nagents_env
    R = E * N
    assert ops.bptt_passes_backward_supported(env, H, P) and not ops.bptt_passes_backward_supported(env, H, 1)
    w = ref.make_window(sum(map(ord, name)), T, E, N, H, OT, P, share=cfg.get('share', False), alive=cfg.get('alive', 'none'))
    snaps, obs = _snapshots(env, T)
    want = ref.reference_of(w, obs=obs, detach_gap=cfg.get('gap', 0), mode_avg=cfg.get('avg', True), comm_zero=cfg.get('comm_zero', False))
    got = _launch(env, w, cfg, snaps)
    num = lambda v: v.double().cpu().numpy()
    errs = dict(dgates=ref.rel_err(num(got['gates']), want['dgates']), dxh=ref.rel_err(num(got['dxh']), want['dxh']),
                dh=ref.rel_err(num(got['dh']), want['dh']), dc=ref.rel_err(num(got['dc']), want['dc']),
                dbias_rows=ref.rel_err(num(got['bias']), num(got['bias0']) + want['dbias_rows']))
    if cfg.get('comm_zero', False):
        assert torch.equal(got['dcw'].cpu(), got['dcw0'])
    else:
        errs['dcw'] = ref.rel_err(num(got['dcw']).sum(1), num(got['dcw0']).sum(1) + want['dcw'])
    errs['dcb'] = ref.rel_err((num(got['bias']) - num(got['bias0'])).sum(1) @ w['w_ih'].astype(np.float64), want['dcb'])
    dwt, db = env.encode_backward_window_finish(H)
    errs['enc_dwt'], errs['enc_db'] = ref.rel_err(num(dwt), want['enc_dwt']), ref.rel_err(num(db), want['enc_db'])
    dW0 = torch.randn((2 * H, 4 * H), generator=torch.Generator().manual_seed(5))
    dW = dW0.to(dev)
    up = lambda a: torch.from_numpy(a).to(dev)
    ops.lstm_weight_grad(up(w['inp']).reshape(P * T * R, H), up(w['hs']).reshape(P * T * R, H), got['gates'], dW)
    errs['dW'] = ref.rel_err(num(dW), num(dW0) + want['dW'])
    again = _launch(env, w, cfg, snaps)
    for k in ('gates', 'dh', 'dc', 'bias', 'dcw'):
        assert torch.equal(got[k], again[k]), k
    ref.check('gpu/' + name, errs)


def test_a_refused_window_leaves_the_records_alone():
    """A pass without its ring (a NULL entry in the host array): ValueError naming the pass, before any launch — gates, dh, dc and the
    partials keep their bits, the other rings stay unwritten."""
    import ctypes as C
    from ic3net_amd import _lib, ops
    env = _pp(3, 6, 1, 130)
    dev = env.device
    T, E, N, H, P = 2, 130, 3, 64, 2
    R = E * N
    w = ref.make_window(1, T, E, N, H, OT, P)
    snaps, _ = _snapshots(env, T)
    up = lambda a: torch.from_numpy(a).to(dev)
    gates, hs, cs, dh, dc, dhead = up(w['gates']), up(w['hs']), up(w['cs']), up(w['dh']), up(w['dc']), up(w['dhead'])
    dxh = torch.full((P, T, R, 2 * H), float('nan'), device=dev)
    bias = torch.ones((P, (R + 63) // 64, 4 * H), device=dev)
    dcw = torch.ones((P, ops.comm_backward_partials(E, N), H, H), device=dev)
    wb3 = ops.policy_pack_split_bwd(up(w['w_ih']), up(w['w_hh']))
    w_heads, cws, gt = up(w['w_heads']), [up(a) for a in w['c_weights']], [up(m) for m in w['gate']]
    arr = lambda ts: C.cast((C.c_void_p * len(ts))(*[None if t is None else t.data_ptr() for t in ts]), C.POINTER(C.c_void_p))
    b = _lib.BpttPasses(T, E, N, H, OT, P, 1, 0, 0, 1, 0)
    b.gates, b.hs, b.cs = arr([gates[0], gates[1]]), arr([hs[0], hs[1]]), arr([cs[0], cs[1]])
    b.dxh, b.dbias_partials, b.dcw_partials = arr([dxh[0], None]), arr([bias[0], bias[1]]), arr([dcw[0], dcw[1]])
    b.c_weight, b.gate = arr(cws), arr(gt)
    b.dhead, b.snaps, b.snap_words = dhead.data_ptr(), snaps.data_ptr(), snaps.stride(0)
    b.lstm_wp3_bwd, b.w_heads, b.dh, b.dc = wb3.data_ptr(), w_heads.data_ptr(), dh.data_ptr(), dc.data_ptr()
    b.dxh_step, b.enc_work = R * 2 * H, env.encode_window_work(H).data_ptr()
    with pytest.raises(ValueError, match="pass 1"):
        _lib.check(_lib.lib().ic3_bptt_backward(env._h, C.byref(b), _lib.stream()))
    torch.cuda.synchronize()
    assert torch.equal(gates.cpu(), torch.from_numpy(w['gates'])) and torch.equal(dh.cpu(), torch.from_numpy(w['dh']))
    assert torch.equal(dc.cpu(), torch.from_numpy(w['dc'])) and bool((bias == 1).all()) and bool((dcw == 1).all())
    assert bool(torch.isnan(dxh).all())


def test_chunked_window_driver_against_the_unchunked_run_and_float64():
    """h64-pp-n3-E130-T5-P2-chunk2: bptt._backward_window_multipass on a synthetic record (random (h, c) entering every step, random
    gate masks, real snapshots) with max_chunk_steps = 2 — chunks of 2, 2 and 1 steps, last first — against the same window in one
    chunk: dgates of every (t, i), dh and dc leaving the window the same bits (the detach points, the carried dh / dc and the masks
    land on the same steps); and the chunked run against float64 (the passes re-evaluated from the recorded state of every step,
    then the window backward): dgates, dh, dc and every gradient the driver adds to its accumulators, each at its bar."""
    import bench
    from ic3net_amd import bptt
    name = 'h64-pp-n3-E130-T5-P2-chunk2'
    E, T, P, H, gap = 130, 5, 2, 64, 2
    tr, a = bench.build_trainer("pp_easy", E, 3, 0, 0, comm_passes=P, hid_size=H)
    a.detach_gap = gap
    net, raw = tr._kernel_net(), tr.env.env
    assert net is tr.policy_net
    N = a.nagents
    R = E * N
    dev = raw.device
    rng = np.random.default_rng(sum(map(ord, name)))
    f32 = lambda x: np.ascontiguousarray(x, np.float32)
    snaps, obs = _snapshots(raw, T)
    rec = bptt.EpisodeRecord(T, R, H, raw.dims.state_words, dev)
    hs, cs = f32(np.tanh(rng.standard_normal((T + 1, R, H)))), f32(rng.standard_normal((T + 1, R, H)))
    rec.hs.copy_(torch.from_numpy(hs))
    rec.cs.copy_(torch.from_numpy(cs))
    rec.snaps.copy_(snaps)
    gate = [np.ascontiguousarray(rng.random((E, N)) < 0.6, np.int32) for _ in range(T)]
    rec.gate = [torch.from_numpy(m).to(dev) for m in gate]
    rec.n, rec.h_last = T, rec.hs[T]
    OTn = sum(a.naction_heads) + 1
    dhead = f32(rng.standard_normal((T, R, OTn)))
    d_out = torch.from_numpy(dhead).to(dev)
    assert bptt._multipass_window_ok(a, net, raw, rec, d_out)

    def run(most):
        acc = bptt.new_accumulators(net)
        dgates = torch.full((P, T, R, 4 * H), float('nan'), device=dev)
        with torch.no_grad():
            dh, dc = bptt._backward_window_multipass(a, net, raw, rec, d_out, acc, max_chunk_steps=most, dgates_out=dgates)
        torch.cuda.synchronize()
        return dict(dgates=dgates, dh=dh, dc=dc, acc=acc, chunk=net.multipass_window_chunk)
    whole, chunked = run(0), run(2)
    assert whole['chunk'] == T and chunked['chunk'] == 2
    for k in ('dgates', 'dh', 'dc'):
        assert torch.equal(whole[k], chunked[k]), k
    sd = {k: v.detach().double().cpu().numpy() for k, v in net.state_dict().items()}
    x = np.stack([o @ sd['encoder.weight'].T + sd['encoder.bias'] for o in obs])
    cws, cbs = [sd['C_modules.%d.weight' % i] for i in range(P)], [sd['C_modules.%d.bias' % i] for i in range(P)]
    w_ih, w_hh = sd['f_module.weight_ih'], sd['f_module.weight_hh']
    fwd = ref.window_forward(x, None, None, cws, cbs, w_ih, w_hh, sd['f_module.bias_ih'] + sd['f_module.bias_hh'], E, N, gate=gate,
                             entering=(hs, cs))
    nh = len(a.naction_heads)
    w_heads = np.concatenate([sd['heads.%d.weight' % k] for k in range(nh)] + [sd['value_head.weight']], 0)
    want = ref.window_backward(fwd['gates'], fwd['hs'], fwd['cs'], dhead, w_heads, w_ih, w_hh, np.zeros((R, H)), np.zeros((R, H)), E, N,
                               c_weights=cws, gate=gate, detach_gap=gap, obs=obs, inp=fwd['inp'])
    num = lambda v: v.double().cpu().numpy()
    acc = chunked['acc']
    errs = dict(dgates=ref.rel_err(num(chunked['dgates']), want['dgates']), dh=ref.rel_err(num(chunked['dh']), want['dh']),
                dc=ref.rel_err(num(chunked['dc']), want['dc']), dW=ref.rel_err(num(acc['w_cat_t']), want['dW']),
                dbias=ref.rel_err(num(acc['b_cat']), want['dbias_rows'].sum((0, 1))),
                dcw=ref.rel_err(np.stack([num(g) for g in acc['c_w_p']]), want['dcw']),
                dcb=ref.rel_err(np.stack([num(g) for g in acc['c_b']]), want['dcb']),
                enc_dwt=ref.rel_err(num(acc['wt']), want['enc_dwt']), enc_db=ref.rel_err(num(acc['enc_bias']), want['enc_db']))
    ref.check('gpu/' + name, errs)
