"""GPU: what the wrappers of ic3net_amd/ops.py accept and what they refuse — one valid tiny call per wrapper family on a Predator-Prey
env (E = 2, N = 3, dim 5, vision 0, hid 64, T = 2, OT = 6): finite outputs of the documented shapes; then the same call with ONE
argument spoiled (a float mask, a buffer that is not contiguous, an (R, H + 1) carry, a short `snaps`, a CPU tensor) and the
exception type it raises.  Every refusal asserted here is raised on the host before any launch: by _need_cuda (IC3Error), by an
assert of the wrapper (AssertionError), or by the library's own argument validation, which runs before its first launch
(ValueError: ic3_bptt_backward's detach_gap + row_keep, ic3_episode_scratch_bytes answering 0)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

E, N, H, T, HEADS = 2, 3, 64, 2, (5,)
R, OT = E * N, sum(HEADS) + 1


class Ctx(object):
    def __init__(self):
        from test_env_parity_gpu import make_pp
        from ic3net_amd import ops
        self.env = env = make_pp(N, 5, 0, 'mixed', E, seed=3)
        self.dev = env.device
        self.gen = torch.Generator(device=self.dev).manual_seed(11)
        env.reset()
        self.snaps = torch.empty((T, env.dims.state_words), dtype=torch.int32, device=self.dev)
        for t in range(T):
            env.step(torch.full((E, N), t + 1, dtype=torch.int32, device=self.dev), observe=False)
            env.snapshot(out=self.snaps[t])
        self.w_ih, self.w_hh = self.rn(4 * H, H) * 0.1, self.rn(4 * H, H) * 0.1
        self.cw, self.fw = self.rn(H, H) * 0.1, self.rn(H, H) * 0.1
        self.wt, self.enc_bias = self.rn(env.obs_dim, H) * 0.1, self.rn(H) * 0.1
        self.w_heads, self.b_heads = self.rn(OT, H) * 0.1, self.rn(OT) * 0.1
        self.fc = dict(wt=self.wt, enc_bias=self.enc_bias, loc_table=None, b_cat=self.rn(4 * H) * 0.1, w_heads=self.w_heads,
                       b_heads=self.b_heads, ps_l_wp3=ops.policy_pack_split(self.w_ih, self.w_hh))
        self.fc.update(ops.policy_step_pack(self.cw, self.w_ih, self.w_hh))
        self.wb3 = ops.policy_pack_split_bwd(self.w_ih, self.w_hh)
        zb = [torch.zeros(H, device=self.dev)]
        wp, bias = ops.commnet_pack([self.cw], [self.fw], zb, zb)
        self.cn = dict(wt=self.wt, enc_bias=self.enc_bias, loc_table=None, wp=wp, bias=bias, w_heads=self.w_heads, b_heads=self.b_heads,
                       wp3=ops.commnet_pack_split([self.cw], [self.fw]))

    def rn(self, *shape):
        return torch.randn(*shape, device=self.dev, generator=self.gen)

    def unit(self, *shape):                                      # (0.1, 0.9): activated gates, tanh states
        return torch.rand(*shape, device=self.dev, generator=self.gen) * 0.8 + 0.1

    def ones(self, *shape):
        return torch.ones(shape, dtype=torch.int32, device=self.dev)

    def zeros(self, *shape):
        return torch.zeros(shape, device=self.dev)


@pytest.fixture(scope="module")
def ctx():
    return Ctx()


def _finite(*tensors):
    torch.cuda.synchronize()
    return all(bool(torch.isfinite(t).all()) for t in tensors)


# ---- one builder per family: (wrapper, keyword arguments of a valid call, check(kw, returned)) ---------------------------------
def f_comm_masked_mean_raw(c):
    from ic3net_amd import ops
    kw = dict(h=c.rn(E, N, H), alive=c.ones(E, N), comm_action=c.ones(E, N), mode_avg=True, mask_self=True, addend=c.rn(R, H),
              row_scale=c.unit(R))

    def ok(kw, out):
        assert tuple(out.shape) == (E, N, H) and out.dtype == torch.float32 and _finite(out)
    return ops.comm_masked_mean_raw, kw, ok


def f_lstm_gates_backward_given(c):
    from ic3net_amd import ops
    kw = dict(gates=c.unit(R, 4 * H), c_prev=c.rn(R, H), dh=c.rn(R, H), dc=c.rn(R, H), dgates=c.zeros(R, 4 * H), dc_prev=c.zeros(R, H),
              dbias_partials=c.zeros(1, 4 * H))

    def ok(kw, n):
        assert n >= 0 and _finite(kw['dgates'], kw['dc_prev'], kw['dbias_partials']) and float(kw['dgates'].abs().max()) > 0
    return ops.lstm_gates_backward_given, kw, ok


def f_comm_backward(c):
    from ic3net_amd import ops
    kw = dict(dxh=c.rn(R, 2 * H), h_prev=c.rn(R, H), alive=c.ones(E, N), gate=c.ones(E, N), c_weight=c.cw, dh_out=c.zeros(R, H),
              dcw_partials=c.zeros(ops.comm_backward_partials(E, N), H, H), E=E, N=N)

    def ok(kw, n):
        assert n >= 0 and _finite(kw['dh_out'], kw['dcw_partials']) and float(kw['dh_out'].abs().max()) > 0
    return ops.comm_backward, kw, ok


def f_bptt_backward(c):
    from ic3net_amd import ops
    assert ops.bptt_backward_supported(c.env, H)
    kw = dict(env=c.env, T=T, E=E, N=N, H=H, gates=c.unit(T, R, 4 * H), hs=c.rn(T, R, H), cs=c.rn(T, R, H), dhead=c.rn(T, R, OT),
              snaps=c.snaps, alive=None, gate=[c.ones(E, N) for _ in range(T)], lstm_wp3_bwd=c.wb3, w_heads=c.w_heads, c_weight=c.cw,
              dh=c.rn(R, H), dc=c.rn(R, H), dxh=c.zeros(T, R, 2 * H), dbias_partials=c.zeros(1, 4 * H),
              dcw_partials=c.zeros(ops.bptt_dcw_partials(E, N, False), H, H))

    def ok(kw, ret):
        assert ret is None and _finite(kw['gates'], kw['dh'], kw['dc'], kw['dxh'], kw['dbias_partials'], kw['dcw_partials'])
        assert tuple(kw['dxh'].shape) == (T, R, 2 * H) and float(kw['dxh'].abs().max()) > 0
    return ops.bptt_backward, kw, ok


def f_rnn_backward(c):
    from ic3net_amd import ops
    assert ops.rnn_backward_supported(c.env, H)
    kw = dict(env=c.env, T=T, E=E, N=N, H=H, hs=c.unit(T + 1, R, H), dhead=c.rn(T, R, OT), snaps=c.snaps, a2=c.fw, w_heads=c.w_heads,
              dh=c.rn(R, H), dz=c.zeros(T, R, H), dbias_partials=c.zeros(ops.rnn_backward_partials(R, H), H), a2_grad=c.zeros(H, H))

    def ok(kw, ret):
        assert ret is None and _finite(kw['dh'], kw['dz'], kw['dbias_partials'], kw['a2_grad']) and float(kw['dz'].abs().max()) > 0
    return ops.rnn_backward, kw, ok


def f_mlp_backward(c):
    from ic3net_amd import ops
    assert ops.mlp_backward_supported(c.env, H)
    kw = dict(env=c.env, T=T, E=E, N=N, H=H, h=c.unit(T, R, H), dhead=c.rn(T, R, OT), snaps=c.snaps, enc_wt=c.wt, enc_bias=c.enc_bias,
              a2=c.fw, w_heads=c.w_heads, x1=c.zeros(T, R, H), dz=c.zeros(T, R, H), de=c.zeros(T, R, H),
              dbias_partials=c.zeros(ops.mlp_backward_partials(T * R, H), H), a2_grad=c.zeros(H, H))

    def ok(kw, ret):
        assert ret is None and _finite(kw['x1'], kw['dz'], kw['de'], kw['dbias_partials'], kw['a2_grad'])
        assert float(kw['de'].abs().max()) > 0
    return ops.mlp_backward, kw, ok


def f_commnet_backward(c):
    from ic3net_amd import ops
    assert ops.commnet_backward_supported(c.env, H, N)
    kw = dict(env=c.env, T=T, E=E, N=N, H=H, dhead=c.rn(T, R, OT), snaps=c.snaps, alive=c.ones(T, E, N), gate=c.ones(T, E, N),
              enc_wt=c.wt, enc_bias=c.enc_bias, wp=c.cn['wp'], bias=c.cn['bias'], w_heads=c.w_heads, f_weights=[c.fw], c_weights=[c.cw],
              f_grads=[c.zeros(H, H)], c_grads=[c.zeros(H, H)], bias_grads=[c.zeros(H)], heads_w_grad=c.zeros(OT, H),
              heads_b_grad=c.zeros(OT), wp3=c.cn['wp3'], work={})

    def ok(kw, ret):
        rings, chunks = ret
        assert chunks >= 1 and set(rings) == {'h_pass', 'dxh', 'dz', 'dx', 'de', 'dh'}
        Qc = rings['dz'].shape[0]
        assert Qc % R == 0 and tuple(rings['h_pass'].shape) == (2, Qc, H) and tuple(rings['dxh'].shape) == (Qc, 2 * H)
        assert _finite(kw['f_grads'][0], kw['c_grads'][0], kw['bias_grads'][0], kw['heads_w_grad'], kw['heads_b_grad'], *rings.values())
        assert float(kw['f_grads'][0].abs().max()) > 0
    return ops.commnet_backward, kw, ok


def _step_outputs(c):
    return dict(out=c.zeros(R, OT), action=torch.zeros((len(HEADS), E, N), dtype=torch.int32, device=c.dev), reward=c.zeros(E, N),
                done=torch.zeros((E,), dtype=torch.int32, device=c.dev))


def f_policy_step(c):
    from ic3net_amd import ops
    assert ops.policy_step_supported(c.env, H)
    c.env.reset()
    kw = dict(env=c.env, fc=c.fc, H=H, head_sizes=HEADS, mode_avg=True, comm_zero=False, h=c.zeros(R, H), c=c.zeros(R, H),
              alive_in=None, comm_in=c.ones(E, N), **_step_outputs(c))

    def ok(kw, out):
        assert out is kw['out'] and _finite(out, kw['h'], kw['c'], kw['reward'])
        assert torch.allclose(out[:, :5].exp().sum(1), torch.ones(R, device=out.device), atol=1e-5)      # log-probs of the head
        assert int(kw['action'].min()) >= 0 and int(kw['action'].max()) < 5
    return ops.policy_step, kw, ok


def f_commnet_step(c):
    from ic3net_amd import ops
    assert ops.commnet_step_supported(c.env, H)
    c.env.reset()
    kw = dict(env=c.env, cn=c.cn, H=H, head_sizes=HEADS, mode_avg=True, comm_zero=False, alive_in=c.ones(E, N), comm_in=None,
              **_step_outputs(c))

    def ok(kw, out):
        assert out is kw['out'] and _finite(out, kw['reward'])
        assert torch.allclose(out[:, :5].exp().sum(1), torch.ones(R, device=out.device), atol=1e-5)
        assert int(kw['action'].min()) >= 0 and int(kw['action'].max()) < 5
    return ops.commnet_step, kw, ok


def f_episode_finalize(c):
    from ic3net_amd import ops
    done = torch.zeros((T, E), dtype=torch.int32, device=c.dev)
    done[T - 1] = 1
    kw = dict(done=done, reward=c.rn(T, E, N), alive=c.ones(T, E, N), is_completed=torch.zeros((T, E, N), dtype=torch.int32, device=c.dev))

    def ok(kw, res):
        shapes = dict(live=(T, E), alive_mask=(T, E, N), episode_mask=(T, E), episode_mini_mask=(T, E, N), live_after=(E,),
                      stats=(2 + 2 * N,))
        assert {k: tuple(v.shape) for k, v in res.items()} == shapes and res['stats'].dtype == torch.float64
        assert _finite(*res.values())
    return ops.episode_finalize, kw, ok


def f_loss_gradients(c):
    from ic3net_amd import ops
    out = torch.cat([torch.log_softmax(c.rn(T, R, 5), -1), c.rn(T, R, 1)], -1).contiguous()
    kw = dict(out=out, action=torch.ones((T, len(HEADS), R), dtype=torch.int32, device=c.dev), returns=c.rn(T, R),
              alive_mask=torch.ones((T, R), device=c.dev), live=torch.ones((T, E), device=c.dev), head_sizes=HEADS, entr=0.01,
              value_coeff=0.05)

    def ok(kw, ret):
        d_out, sums = ret
        assert tuple(d_out.shape) == (T, R, OT) and tuple(sums.shape) == (3,) and sums.dtype == torch.float64 and _finite(d_out, sums)
    return ops.loss_gradients, kw, ok


def f_heads_grad(c):
    from ic3net_amd import ops
    kw = dict(d=c.rn(T * R, OT), h=c.rn(T * R, H), dW=c.zeros(OT, H), db=c.zeros(OT))

    def ok(kw, ret):
        assert ret is None and _finite(kw['dW'], kw['db'])
        torch.testing.assert_close(kw['db'], kw['d'].sum(0), rtol=1e-5, atol=1e-5)
    return ops.heads_grad, kw, ok


FAMILIES = dict(comm_masked_mean_raw=f_comm_masked_mean_raw, lstm_gates_backward_given=f_lstm_gates_backward_given,
                comm_backward=f_comm_backward, bptt_backward=f_bptt_backward, rnn_backward=f_rnn_backward, mlp_backward=f_mlp_backward,
                commnet_backward=f_commnet_backward, policy_step=f_policy_step, commnet_step=f_commnet_step,
                episode_finalize=f_episode_finalize, loss_gradients=f_loss_gradients, heads_grad=f_heads_grad)


@pytest.mark.parametrize("family", list(FAMILIES))
def test_a_valid_call(ctx, family):
    fn, kw, ok = FAMILIES[family](ctx)
    ok(kw, fn(**kw))


# ---- the spoilings --------------------------------------------------------------------------------------------------------------
def _each(v, f):
    return [f(m) for m in v] if isinstance(v, list) else f(v)


SPOIL = dict(
    float=lambda v: _each(v, lambda t: t.float()),                                          # a float mask
    strided=lambda v: torch.stack([v, v], -1)[..., 0],                                      # same shape and values, not contiguous
    wider=lambda v: torch.zeros(v.shape[:-1] + (v.shape[-1] + 1,), dtype=v.dtype, device=v.device),     # (.., H + 1)
    short=lambda v: v[:-1],                                                                 # one snapshot too few
    cpu=lambda v: v.cpu(),
)


def _refusals():
    from ic3net_amd._lib import IC3Error
    A = AssertionError
    return [
        ('comm_masked_mean_raw', 'row_scale', 'strided', A), ('comm_masked_mean_raw', 'h', 'cpu', IC3Error),
        ('lstm_gates_backward_given', 'dgates', 'strided', A), ('lstm_gates_backward_given', 'c_prev', 'wider', A),
        ('lstm_gates_backward_given', 'gates', 'cpu', IC3Error),
        ('comm_backward', 'alive', 'float', A), ('comm_backward', 'dxh', 'strided', A), ('comm_backward', 'dh_out', 'wider', A),
        ('comm_backward', 'dxh', 'cpu', IC3Error),
        ('bptt_backward', 'gate', 'float', A), ('bptt_backward', 'snaps', 'short', A), ('bptt_backward', 'dh', 'wider', A),
        ('bptt_backward', 'dhead', 'strided', A), ('bptt_backward', 'gates', 'cpu', IC3Error),
        ('rnn_backward', 'snaps', 'short', A), ('rnn_backward', 'dh', 'wider', A), ('rnn_backward', 'dz', 'strided', A),
        ('rnn_backward', 'hs', 'cpu', IC3Error),
        ('mlp_backward', 'snaps', 'short', A), ('mlp_backward', 'enc_wt', 'strided', A), ('mlp_backward', 'x1', 'wider', A),
        ('mlp_backward', 'h', 'cpu', IC3Error),
        ('commnet_backward', 'alive', 'float', A), ('commnet_backward', 'snaps', 'short', A), ('commnet_backward', 'wp', 'strided', A),
        ('commnet_backward', 'dhead', 'cpu', IC3Error),
        ('policy_step', 'comm_in', 'float', A), ('policy_step', 'h', 'wider', A), ('policy_step', 'out', 'strided', A),
        ('policy_step', 'h', 'cpu', IC3Error),
        ('commnet_step', 'alive_in', 'float', A), ('commnet_step', 'action', 'float', A), ('commnet_step', 'out', 'strided', A),
        ('commnet_step', 'out', 'cpu', IC3Error),
        ('episode_finalize', 'alive', 'float', A), ('episode_finalize', 'done', 'strided', A), ('episode_finalize', 'reward', 'cpu', IC3Error),
        ('loss_gradients', 'action', 'float', A), ('loss_gradients', 'returns', 'strided', A), ('loss_gradients', 'out', 'cpu', IC3Error),
        ('heads_grad', 'd', 'strided', A), ('heads_grad', 'dW', 'wider', A), ('heads_grad', 'd', 'cpu', IC3Error),
    ]


REFUSALS = [r[:3] for r in _refusals()]


@pytest.mark.parametrize("family,arg,how", REFUSALS, ids=["%s-%s-%s" % r for r in REFUSALS])
def test_a_spoiled_argument_is_refused_on_the_host(ctx, family, arg, how):
    exc = {r[:3]: r[3] for r in _refusals()}[(family, arg, how)]
    fn, kw, ok = FAMILIES[family](ctx)
    bad = SPOIL[how](kw[arg])
    if how == 'strided':
        assert not bad.is_contiguous() and bad.shape == kw[arg].shape
    with pytest.raises(exc) as info:
        fn(**dict(kw, **{arg: bad}))
    assert type(info.value) is exc                               # (the type itself, not a subclass of it)


def test_refusals_of_the_library_before_its_first_launch(ctx):
    """ValueError, as the wrappers answer -22 of the library: ic3_bptt_backward refuses detach_gap > 0 together with row_keep before
    its first launch (the record keeps its bits: tests/test_bptt_window_gpu.py); episode_finalize refuses sizes ic3_episode_scratch_bytes
    has no layout for."""
    from ic3net_amd import ops
    fn, kw, ok = f_bptt_backward(ctx)
    before = kw['gates'].clone()
    with pytest.raises(ValueError, match="detach_gap.*row_keep"):
        fn(**dict(kw, detach_gap=1, row_live=torch.ones((T, R), device=ctx.dev), row_keep=torch.ones((T, R), device=ctx.dev)))
    torch.cuda.synchronize()
    assert torch.equal(kw['gates'], before)
    with pytest.raises(ValueError):
        ops.episode_finalize(torch.zeros((1, 2), dtype=torch.int32, device=ctx.dev), torch.zeros((1, 2, 300), device=ctx.dev))
