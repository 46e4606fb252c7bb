"""CPU: the replay hook of the simulation tests (rmc_selftest_replay_binds).

The GPU tests (test_gpu_simulate_oracle.py) turn a walker's recorded bindings
into states through this hook.  Here, without a GPU: a chain of enabled
bindings loads as a behaviour the oracle replays, and a chain with a binding
that is not enabled is an error (RaftmcError carrying rmc_last_error), never
an abort, and leaves the model usable.
"""
import json
import os

import pytest

import raftmc
from oracle.pyoracle import make_spec, parse_cfg
from test_trace_module import parse_trace_states, replay_with_oracle

HERE = os.path.dirname(os.path.abspath(__file__))
SMALL = json.load(open(os.path.join(HERE, "golden", "small.json")))


def _enabled_chain(m, length):
    """Greedy: extend the chain by the lowest binding the hook accepts."""
    chain = []
    for _ in range(length):
        for b in range(256):
            try:
                m.selftest_replay_binds(chain + [b])
            except raftmc.RaftmcError:
                continue
            chain.append(b)
            break
        else:
            break
    return chain


@pytest.mark.parametrize("name", ["raft_n3v1e1r1", "pull_n2v1e2r1"])
def test_replay_binds_loads_a_behaviour_and_rejects_disabled_bindings(name):
    g = SMALL[name]
    m = raftmc.Model(module=g["module"], cfg_text=g["cfg"])
    spec = make_spec(g["module"], parse_cfg(g["cfg"]))
    assert m.selftest_replay_binds([]) == 1  # Init alone
    chain = _enabled_chain(m, 4)
    assert len(chain) == 4
    disabled_in_init = [b for b in range(256) if b not in _enabled_first(m)]
    assert m.selftest_replay_binds(chain) == 5
    states = parse_trace_states(m.trace_module(g["module"] + "_STrace")[0])
    assert len(states) == 5
    replay_with_oracle(spec, states)
    # not enabled in its state: a binding Init does not enable, a binding past
    # every table, and enabled steps followed by one that is not
    for bad in ([disabled_in_init[0]], [0xFFFF], chain[:2] + [0xFFFF], chain + [60000]):
        with pytest.raises(raftmc.RaftmcError, match="not enabled"):
            m.selftest_replay_binds(bad)
    # the failed calls left the last loaded behaviour in place, and the model works
    assert parse_trace_states(m.trace_module(g["module"] + "_STrace")[0]) == states
    assert m.selftest_replay_binds(chain[:1]) == 2


def _enabled_first(m):
    out = []
    for b in range(256):
        try:
            m.selftest_replay_binds([b])
            out.append(b)
        except raftmc.RaftmcError:
            pass
    return out
