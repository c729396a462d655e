"""CPU: the ctypes binding itself (ic3net_amd/_lib.py, the shared helpers of ops.py) — struct layouts, what the sized structs fill
in at construction, the argument predicates, the row-stride helper and ops._policy_struct byte for byte.  No GPU, and the library is
never loaded."""
import ctypes as C

import pytest
import torch

from ic3net_amd import _lib, ops

# name: (ctypes.sizeof, the field names in order) as include/ic3_rollout.h lays the structs out (ABI 601)
LAYOUT = {
    'PPCfg': (44, 'E N nprey dim vision mode stay moving_prey enemy_comm seed env_id_offset'),
    'TJCfg': (64, 'E N dim vision difficulty vocab_type add_rate_min add_rate_max curr_start curr_end seed env_id_offset'),
    'Dims': (52, 'kind E N obs_dim vocab naction window npath narrival max_route_len grid_h grid_w state_words'),
    'Stats': (56, 'success_sum add_rate episodes live_env_steps auto_success_sum auto_episodes auto_env_steps'),
    'Policy': (192, 'struct_size H nheads head_sizes mode_avg comm_zero enc_wt enc_bias loc_table c_wp lstm_wp lstm_bias head_w head_b '
                    'pass_index inner_pass gate_split npasses lstm_wp3 c_wp_pass enc_bias_pass'),
    'Episode': (144, 'struct_size n E N auto_reset forced_last gate_ones done alive is_completed reward gate gate_stride live alive_mask '
                     'episode_mask episode_mini_mask live_after stats scratch counter'),
    'Bptt': (216, 'struct_size T E N H OT mode_avg comm_zero detach_gap enc_first gates hs cs dhead snaps snap_words alive gate row_live '
                  'row_keep lstm_wp3_bwd w_heads c_weight dh dc dxh dbias_partials dcw_partials enc_work dxh_step two_chains gate_events'),
    'RnnBptt': (160, 'struct_size T E N H OT detach_gap enc_first enc_window hs h_last dhead snaps snap_words a2 w_heads row_live row_keep '
                     'dh dz dbias_partials enc_work a2_grad wgrad_scratch'),
    'MlpBptt': (160, 'struct_size T E N H OT enc_first enc_window h dhead snaps snap_words enc_wt enc_bias loc_table a2 w_heads x1 dz de '
                     'dbias_partials enc_work a2_grad wgrad_scratch'),
    'CommnetBptt': (264, 'struct_size T E N H OT passes mode_avg comm_zero enc_first enc_window max_chunk_steps dhead snaps snap_words '
                         'alive gate enc_wt enc_bias loc_table wp wp3 bias w_heads f_weight c_weight f_grad c_grad bias_grad heads_w_grad '
                         'heads_b_grad h_pass dxh dz dx de dh scratch enc_work'),
}
SIZED = ['Policy', 'Episode', 'Bptt', 'RnnBptt', 'MlpBptt', 'CommnetBptt']


@pytest.mark.parametrize("name", list(LAYOUT))
def test_struct_layout(name):
    size, fields = LAYOUT[name]
    cls = getattr(_lib, name)
    assert C.sizeof(cls) == size
    assert [f[0] for f in cls._fields_] == fields.split()


@pytest.mark.parametrize("name", SIZED)
def test_sized_structs_fill_their_size(name):
    cls = getattr(_lib, name)
    s = cls()
    assert s.struct_size == C.sizeof(cls) == LAYOUT[name][0]
    assert bytes(s)[4:] == bytes(C.sizeof(cls) - 4)              # everything behind it zero
    s.struct_size = 7                                            # (a caller may still overwrite it: tests/test_abi_cpu.py)
    assert s.struct_size == 7


def test_positional_arguments_start_behind_struct_size():
    ep = _lib.Episode(4, 2, 3, 0, 0, 0)
    assert (ep.n, ep.E, ep.N) == (4, 2, 3) and ep.struct_size == 144
    b = _lib.Bptt(5, 2, 3, 64, 6, 1, 0, 2, 1)
    assert (b.T, b.E, b.N, b.H, b.OT, b.mode_avg, b.comm_zero, b.detach_gap, b.enc_first) == (5, 2, 3, 64, 6, 1, 0, 2, 1)
    assert b.struct_size == 216 and _lib.Policy(H=64).H == 64


def test_exports_and_version():
    assert len(_lib.EXPORTS) == 110 and _lib.ABI_VERSION == 601


def test_int32_array():
    a = _lib.int32_array([5, 2.0])
    assert a._type_ is C.c_int32 and list(a) == [5, 2]
    assert list(_lib.int32_array((5, 2), 4)) == [5, 2, 0, 0]
    with pytest.raises(IndexError):
        _lib.int32_array([1] * 5, 4)
    assert _lib.ptr(None) is None


def test_float32_predicate():
    t = torch.zeros(6, 8)
    assert ops._f32(t) and ops._f32(t, (6, 8)) and ops._f32(t, 48) and ops._f32(None, (6, 8), none_ok=True)
    assert not ops._f32(None, (6, 8))                            # None where the argument is required
    assert not ops._f32(t.double(), (6, 8))                      # dtype
    assert not ops._f32(torch.zeros(6, 16)[:, :8], (6, 8))       # a view that is not contiguous
    assert not ops._f32(t, (6, 9)) and not ops._f32(t, (48,)) and not ops._f32(t, 47)      # shape, element count
    assert ops._dense(t.double(), (6, 8)) and not ops._dense(torch.zeros(8, 6).t(), (6, 8))    # any dtype: contiguous of this shape


def test_mask_predicate():
    m = torch.zeros(2, 3, dtype=torch.int32)
    assert ops._mask(m, 6) and ops._mask(None, 6)
    assert not ops._mask(None, 6, none_ok=False)
    assert not ops._mask(m.float(), 6) and not ops._mask(m.long(), 6)                      # dtype
    assert not ops._mask(torch.zeros(2, 6, dtype=torch.int32)[:, ::2], 6)                  # not contiguous
    assert not ops._mask(m, 5) and not ops._mask(m, 7)                                     # rows


def _same_storage(a, b):
    return a.untyped_storage().data_ptr() == b.untyped_storage().data_ptr()


def test_rows():
    """ops._rows: (shape handed to the kernel, row stride, storage shared with the argument)."""
    t = torch.zeros(2, 3, 8)
    k, ld = ops._rows(t, 8)
    assert (tuple(k.shape), ld, _same_storage(k, t)) == ((6, 8), 8, True)
    wide = torch.zeros(6, 20)
    k, ld = ops._rows(wide[:, 4:12], 8)                          # a column slice of a wider row-major buffer
    assert (tuple(k.shape), ld, _same_storage(k, wide)) == ((6, 8), 20, True) and k.data_ptr() == wide[:, 4:12].data_ptr()
    wide3 = torch.zeros(2, 3, 20)
    k, ld = ops._rows(wide3[:, :, 4:12], 8)                      # the same in three dimensions: evenly spaced rows
    assert (tuple(k.shape), ld, _same_storage(k, wide3)) == ((2, 3, 8), 20, True)
    uneven = torch.zeros(2, 5, 20)
    k, ld = ops._rows(uneven[:, :3, 4:12], 8)                    # rows not evenly spaced across dim 0: a copy
    assert (tuple(k.shape), ld, _same_storage(k, uneven), k.is_contiguous()) == ((2, 3, 8), 8, False, True)
    d = torch.zeros(2, 3, 8, dtype=torch.float64)
    k, ld = ops._rows(d, 8)                                      # not float32: converted
    assert (tuple(k.shape), ld, k.dtype, _same_storage(k, d)) == ((6, 8), 8, torch.float32, False)
    tr = torch.arange(48.0).reshape(8, 6).t()
    k, ld = ops._rows(tr, 8)                                     # transposed: made contiguous
    assert (tuple(k.shape), ld, _same_storage(k, tr), k.is_contiguous()) == ((6, 8), 8, False, True) and torch.equal(k, tr)


H, HEADS = 64, (5, 2)


@pytest.fixture(scope="module")
def cache():
    OT = sum(HEADS) + 1
    fc = dict(wt=torch.zeros(29, H), enc_bias=torch.zeros(H), loc_table=torch.zeros(25, H), ps_c_wp=torch.zeros(H * H),
              ps_l_wp=torch.zeros(8 * H * H), b_cat=torch.zeros(4 * H), w_heads=torch.zeros(OT, H), b_heads=torch.zeros(OT))
    for i in (1, 2):
        fc['ps_c_wp_p%d' % i], fc['enc_bias_p%d' % i] = torch.zeros(H * H), torch.zeros(H)
    return fc


def _by_hand(fc, sfx, encoder, split):
    p = _lib.Policy()
    p.struct_size = 192
    p.H, p.nheads = H, 2
    p.head_sizes[0], p.head_sizes[1] = 5, 2
    p.mode_avg, p.comm_zero = 1, 0
    if encoder:
        p.enc_wt, p.enc_bias, p.loc_table = fc['wt'].data_ptr(), fc['enc_bias' + sfx].data_ptr(), fc['loc_table'].data_ptr()
    p.c_wp, p.lstm_wp, p.lstm_bias = fc['ps_c_wp' + sfx].data_ptr(), fc['ps_l_wp'].data_ptr(), fc['b_cat'].data_ptr()
    p.head_w, p.head_b = fc['w_heads'].data_ptr(), fc['b_heads'].data_ptr()
    if split is not None:
        p.gate_split, p.lstm_wp3 = 1, split.data_ptr()
    return p


def test_policy_struct_single_pass(cache):
    want = _by_hand(cache, '', True, None)
    assert bytes(ops._policy_struct(cache, H, HEADS, True, False)) == bytes(want)
    no_table = dict(cache, loc_table=None)
    want.loc_table = None
    assert bytes(ops._policy_struct(no_table, H, HEADS, True, False)) == bytes(want)
    want = _by_hand(cache, '', False, None)                      # ic3_policy_forward: the caller's encoder output
    assert bytes(ops._policy_struct(cache, H, HEADS, True, False, encoder=False)) == bytes(want)


def test_policy_struct_inner_pass(cache):
    want = _by_hand(cache, '_p1', True, None)
    want.pass_index, want.inner_pass = 1, 1
    want.mode_avg, want.comm_zero = 0, 1
    assert bytes(ops._policy_struct(cache, H, HEADS, False, True, pass_index=1, inner=True)) == bytes(want)


def test_policy_struct_three_passes_in_one_launch(cache):
    fc = dict(cache, ps_l_wp3=torch.zeros(24 * H * H, dtype=torch.bfloat16))
    want = _by_hand(fc, '', True, fc['ps_l_wp3'])
    want.npasses = 3
    for i, sf in enumerate(('', '_p1', '_p2')):
        want.c_wp_pass[i], want.enc_bias_pass[i] = fc['ps_c_wp' + sf].data_ptr(), fc['enc_bias' + sf].data_ptr()
    assert bytes(ops._policy_struct(fc, H, HEADS, True, False, passes=3)) == bytes(want)
    with pytest.raises(AssertionError):
        ops._policy_struct(fc, H, HEADS, True, False, passes=3, inner=True)
    with pytest.raises(IndexError):
        ops._policy_struct(fc, H, (2,) * 5, True, False)
