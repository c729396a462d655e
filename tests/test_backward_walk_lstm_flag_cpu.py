"""CPU: the engine flag --backward_walk_lstm (ic3net_amd.main) — known to the parser, an int, off by default, beside --backward_walk,
which keeps its meaning; the binding's BpttWalk against the header's ic3_bptt_walk (its size through the host library's refusal of
another size, the tag's offset and value); and ops.bptt_backward(walk=True) refusing a communicating window in Python, before the
library is touched."""
import ctypes as C
import inspect
import os
import re

import pytest

from ic3net_amd import _lib, main, ops

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'ic3_rollout.h')


def parse(argv):
    argv = ['main.py'] + argv
    return main.build_parser(argv).parse_args(argv[1:])


def test_the_parser_knows_the_flag_and_it_is_off_by_default():
    a = parse([])
    assert a.backward_walk_lstm == 0 and isinstance(a.backward_walk_lstm, int)
    assert a.backward_walk == 0                                                    # no default moved
    a = parse(['--backward_walk_lstm', '1', '--env_name', 'predator_prey'])
    assert a.backward_walk_lstm == 1 and a.backward_walk == 0                      # independent switches
    a = parse(['--backward_walk', '1', '--env_name', 'predator_prey'])
    assert a.backward_walk == 1 and a.backward_walk_lstm == 0
    assert ('backward_walk_lstm', int, 0) in main._ENGINE_FLAGS and ('backward_walk', int, 0) in main._ENGINE_FLAGS


def test_the_binding_struct_is_the_headers():
    """The tag's value is the header's #define and sits where an ic3_bptt holds T; the size differs from both other descriptors of
    ic3_bptt_backward; and the host library, compiled from the header, names its own sizeof when it refuses another one."""
    from host_abi_util import HostEnv, host_lib
    text = open(HEADER).read()
    magic = int(re.search(r"#define\s+IC3_BPTT_WALK_MAGIC\s+(0x[0-9a-fA-F]+)u", text).group(1), 16)
    assert _lib.BpttWalk.MAGIC == magic and magic not in (_lib.BpttPasses.MAGIC, _lib.RnnBpttWalk.MAGIC)
    assert int(re.search(r"#define\s+IC3_VERSION\s+(\d+)", text).group(1)) == 601 == _lib.ABI_VERSION
    assert _lib.BpttWalk.magic.offset == _lib.Bptt.T.offset == 4
    size = C.sizeof(_lib.BpttWalk)
    assert size not in (C.sizeof(_lib.Bptt), C.sizeof(_lib.BpttPasses))
    b = _lib.BpttWalk()
    assert b.struct_size == size and b.magic == magic and b.max_workgroups == 0
    for name in ('alive', 'gate', 'c_weight', 'dcw_partials', 'mode_avg', 'comm_zero', 'two_chains', 'gate_events'):
        assert not hasattr(b, name), name
    lib = host_lib()
    env = HostEnv.pp(3, 6, 1, 'mixed', 4, seed=3)
    b.struct_size = size + 8
    assert lib.ic3_bptt_backward(env._h, C.byref(b), None) == -22
    m = re.match(rb"ic3_bptt_backward \(ic3_bptt_walk\): ic3_bptt_walk has (\d+) bytes, this library's has (\d+)", lib.ic3_last_error())
    assert m and (int(m.group(1)), int(m.group(2))) == (size + 8, size), lib.ic3_last_error()
    env.close()


def test_walk_refuses_a_communicating_window_in_python():
    sig = inspect.signature(ops.bptt_backward).parameters
    assert sig['walk'].default is False and sig['max_workgroups'].default == 0
    nothing = [None] * 15                         # (refused on the flags alone: no tensor, no handle and no library is looked at)
    with pytest.raises(ValueError, match="comm_zero"):
        ops.bptt_backward(None, 2, 4, 3, 64, *nothing, comm_zero=False, walk=True)


def test_walk_refuses_a_window_without_the_ring_in_python():
    import torch
    dxh = torch.zeros((12, 128))                                                   # one buffer, not a ring of T
    args = [None] * 15
    args[12] = dxh
    with pytest.raises(ValueError, match="ring"):
        ops.bptt_backward(None, 2, 4, 3, 64, *args, comm_zero=True, walk=True)
