"""GPU: simulation mode (rmc_simulate -> k_simulate) pinned to the oracle.

A simulation looks random but is a deterministic function of (seed, round,
walker), and the Python oracle gives the exact law of a walk that takes a
uniformly random successor at every step.  So everything the header of
rmc_simulate.cpp promises is checked exactly or against an exact distribution,
on safe configs (the normal use), through two test hooks:
rmc_selftest_simulate_round (one round's launch, returning every walker's
bindings, step count and final row, and replaying every walker on the host)
and rmc_selftest_replay_binds (a binding chain -> the model's trace, so the
trace module turns any walker into states the oracle can replay).

  a. device == host for every walker (every family, KRaft and Variant2 too):
     recorded bindings host-enabled, final rows equal, no behaviour stops
     before a state without successors, no missed invariant failure;
  b. every step of a walker is a Next step of the oracle, its last state has
     no oracle successor, no oracle invariant fails on the way;
  c. the state after t steps follows the exact law of the uniform walk
     (support equal, Pearson chi-square below the 1 - 1e-6 quantile);
  d. generated / depth / behaviors are the sums over the rounds' walkers,
     rounds differ, a partial round is a prefix of the full one;
  e. the step cap cuts behaviours and changes nothing else;
  f. a row out of message slots is reported as capacity overflow.

The fixtures are the smallest that take the restart, fsync, pull,
flexible-quorum and KRaft paths; every uniform walk on them ends in a state
without successors in fewer steps than the fixture's BFS depth, so with
depth = g["depth"] no behaviour is cut by the step cap.
"""
import functools
import json
import os
from fractions import Fraction

import numpy as np
import pytest
from scipy.stats import chi2

import raftmc
from oracle.pyoracle import make_spec, parse_cfg
from test_trace_module import OracleFormatter, parse_trace_states, replay_with_oracle

HERE = os.path.dirname(os.path.abspath(__file__))


def _load(fname):
    with open(os.path.join(HERE, "golden", fname)) as f:
        return json.load(f)


SMALL, KRAFT, VARIANT2 = _load("small.json"), _load("kraft.json"), _load("variant2.json")
# the families OracleFormatter renders (states comparable as TLC value text)
ORACLE = ["raft_n3v1e1r1", "fsync_n2v1e2r1", "pull_n2v1e2r1", "flex_n2v1e2"]
FIX = {n: SMALL[n] for n in ORACLE}
FIX["kraft_n2v1e2"] = KRAFT["kraft_n2v1e2"]
FIX["pull2_n2v1e2r1"] = VARIANT2["pull2_n2v1e2r1"]
SEEDS = [3, 11]
NONE = 0xFFFF  # an unwritten binding slot

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _model(name):
    g = FIX[name]
    return raftmc.Model(module=g["module"], cfg_text=g["cfg"])


@functools.lru_cache(maxsize=None)
def _spec(name):
    g = FIX[name]
    return make_spec(g["module"], parse_cfg(g["cfg"]))


@functools.lru_cache(maxsize=None)
def _round15(name, seed):
    """Round 0 of 1 << 15 walkers at the fixture's depth, replayed on the host
    (shared by tests a and b; nothing mutates it)."""
    r = _model(name).selftest_simulate_round(1 << 15, FIX[name]["depth"], seed=seed)
    for a in (r["binds"], r["steps"], r["rows"]):
        a.setflags(write=False)
    return r


def _masked(binds, steps, t=None):
    """binds[:, :t] with the slots at and after each walker's step count set to NONE."""
    t = binds.shape[1] if t is None else t
    out = binds[:, :t].copy()
    out[np.arange(t)[None, :] >= steps[:, None]] = NONE
    return out


def _live(name, rows):
    """The rows with the words after each one's last message (never written or stale) zeroed."""
    out = rows.copy()
    out[np.arange(rows.shape[1])[None, :] >= (1 + 4 * _spec(name).N + (rows[:, 0] & 0xFF))[:, None]] = 0
    return out


def _no_mismatch(r):
    assert r["mismatch"] == {"binding_not_enabled": (0, 0), "final_row": (0, 0),
                             "stopped_early": (0, 0), "invariant": (0, 0)}, r["mismatch"]


def _successors(spec, s):
    """Next's successors of s, with multiplicity (as a uniform draw over the enabled bindings sees them)."""
    return [t for _, fn in spec.actions() for t in fn(s)]


def _oracle_states(spec, states):
    """replay_with_oracle (asserting every step is a Next step), then the oracle's state of every record."""
    replay_with_oracle(spec, states)
    fmt = OracleFormatter(spec)
    cur = [s for s in spec.init_states() if fmt.state(s) == states[0][1]][0]
    out = [cur]
    for label, want in states[1:]:
        cur = next(t for name, fn in spec.actions() if name.split("(")[0] == label.split("(")[0]
                   for t in fn(cur) if fmt.state(t) == want)
        out.append(cur)
    return out


def _walker_states(name, chain):
    """The behaviour of a binding chain as the trace module's records."""
    m = _model(name)
    n = m.selftest_replay_binds([int(b) for b in chain])
    assert n == len(chain) + 1
    tla, _ = m.trace_module(FIX[name]["module"] + "_STrace")
    states = parse_trace_states(tla)
    assert len(states) == n
    return states


# ---------------------------------------------------------------- a
@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("name", sorted(FIX))
def test_device_walkers_equal_host_replay(name, seed):
    depth = FIX[name]["depth"]
    r = _round15(name, seed)
    assert r["status"] == "ok"
    _no_mismatch(r)
    steps = r["steps"]
    assert 1 <= steps.min() and steps.max() < depth  # every behaviour ends at a state without successors
    # the recorded part of every row is written, nothing after it is
    assert (_masked(r["binds"], steps) != NONE).sum() == steps.sum()
    assert (r["binds"] != NONE).sum() == steps.sum()


# ---------------------------------------------------------------- b
@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("name", ORACLE)
def test_walkers_are_oracle_behaviours(name, seed):
    r = _round15(name, seed)
    spec = _spec(name)
    steps = r["steps"]
    walkers = sorted(set(range(32)) | {int(steps.argmin()), int(steps.argmax())})
    for w in walkers:
        states = _walker_states(name, r["binds"][w, :steps[w]])
        path = _oracle_states(spec, states)
        assert len(path) == steps[w] + 1
        assert _successors(spec, path[-1]) == [], "walker %d stopped at a state with successors" % w
        for k, s in enumerate(path):
            for iname, inv in spec.invariants:
                assert inv(s), "walker %d state %d violates %s" % (w, k + 1, iname)


# ---------------------------------------------------------------- c
@functools.lru_cache(maxsize=None)
def _exact_laws(name, tmax=6):
    """[law after 1 step, ..., after tmax steps] of the uniform-successor walk
    from Init: {state text key: Fraction}.  A state without successors keeps
    its mass."""
    spec = _spec(name)
    fmt = OracleFormatter(spec)
    raw = lambda s: tuple(s[v] for v in spec.variables)
    inits = list(spec.init_states())
    cur = {}
    for s in inits:
        k = raw(s)
        cur[k] = (s, cur.get(k, (s, Fraction(0)))[1] + Fraction(1, len(inits)))
    laws = []
    for _ in range(tmax):
        nxt = {}
        for k, (s, p) in cur.items():
            succ = _successors(spec, s)
            if not succ:
                succ = [s]
            for t in succ:
                kt = raw(t)
                nxt[kt] = (t, nxt.get(kt, (t, Fraction(0)))[1] + p / len(succ))
        cur = nxt
        law = {}
        for s, p in cur.values():
            key = tuple(fmt.state(s)[v] for v in spec.variables)
            law[key] = law.get(key, Fraction(0)) + p
        assert sum(law.values()) == 1
        laws.append(law)
    return laws


def _observed(name, binds, steps, t):
    """{state text key: walkers in that state after t steps}, one host replay per distinct prefix."""
    spec = _spec(name)
    prefixes, counts = np.unique(_masked(binds, steps, t), axis=0, return_counts=True)
    obs = {}
    for pre, c in zip(prefixes, counts):
        chain = pre[pre != NONE]
        fields = _walker_states(name, chain)[-1][1]
        key = tuple(fields[v] for v in spec.variables)
        obs[key] = obs.get(key, 0) + int(c)
    return obs


def _check_law(name, seed, t, law, obs, W):
    cells = len(law)
    min_exp = float(min(law.values()) * W)
    stat = float(sum((obs.get(k, 0) - p * W) ** 2 / (p * W) for k, p in law.items()))
    bound = float(chi2.ppf(1 - 1e-6, cells - 1)) if cells > 1 else 0.0
    print("uniformity %s seed=%d t=%d cells=%d min_expected=%.1f chi2=%.2f quantile=%.2f"
          % (name, seed, t, cells, min_exp, stat, bound))
    assert set(obs) <= set(law), "t=%d: a walker reached a state outside the oracle's support" % t
    assert set(law) <= set(obs), "t=%d: %d states of the oracle's support were never reached" % (t, len(set(law) - set(obs)))
    assert sum(obs.values()) == W
    if cells > 1:
        assert stat < bound, "t=%d: chi-square %.2f over %d cells, bound %.2f" % (t, stat, cells, bound)
    else:
        assert stat == 0


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("name", ORACLE)
def test_successor_draw_follows_exact_law(name, seed):
    W = 1 << 17
    r = _model(name).selftest_simulate_round(W, FIX[name]["depth"], seed=seed, rows=False, host_replay=False)
    assert r["status"] == "ok"
    laws = _exact_laws(name)
    # the largest t <= 6 whose smallest cell still expects 50 walkers
    ok = [t for t in range(1, 7) if min(laws[t - 1].values()) * W >= 50]
    assert ok, "no step with every cell's expected count >= 50"
    for t in sorted({1, max(ok)}):
        _check_law(name, seed, t, laws[t - 1], _observed(name, r["binds"], r["steps"], t), W)


# ---------------------------------------------------------------- d
@pytest.mark.parametrize("name", sorted(FIX))
def test_counters_and_rounds_are_exact(name):
    W, D, seed = 4096, FIX[name]["depth"], 5
    m = _model(name)
    res = m.simulate(walkers=W, behaviors=2 * W + 37, depth=D, seed=seed)
    assert res["status"] == "ok"
    assert res["behaviors"] == 2 * W + 37
    rounds = [m.selftest_simulate_round(W, D, seed=seed, round=k) for k in range(3)]
    for r in rounds:
        assert r["status"] == "ok"
        _no_mismatch(r)
    counted = [rounds[0]["steps"], rounds[1]["steps"], rounds[2]["steps"][:37]]
    assert res["generated"] == res["behaviors"] + sum(int(s.sum(dtype=np.uint64)) for s in counted)
    assert res["depth"] == 1 + max(int(s.max()) for s in counted)
    # the rounds are different behaviours
    b = [_masked(r["binds"], r["steps"]) for r in rounds]
    assert not np.array_equal(b[0], b[1]) and not np.array_equal(b[1], b[2]) and not np.array_equal(b[0], b[2])
    # the partial last round is the first walkers of a full round with its index
    part = m.selftest_simulate_round(37, D, seed=seed, round=2)
    assert part["status"] == "ok"
    _no_mismatch(part)
    assert np.array_equal(part["steps"], rounds[2]["steps"][:37])
    assert np.array_equal(_masked(part["binds"], part["steps"]), b[2][:37])
    assert np.array_equal(_live(name, part["rows"]), _live(name, rounds[2]["rows"][:37]))


# ---------------------------------------------------------------- e
@pytest.mark.parametrize("name", sorted(FIX))
def test_step_cap_and_depth_independence(name):
    W, D, seed, cap = 64, FIX[name]["depth"], 7, 10
    m = _model(name)
    full = m.selftest_simulate_round(W, D, seed=seed)
    _no_mismatch(full)
    assert full["steps"].max() < D
    assert full["steps"].max() > cap  # the cap below cuts some behaviour
    fb = _masked(full["binds"], full["steps"])
    # the API's largest depth: the same behaviours
    big = m.selftest_simulate_round(W, 65535, seed=seed)
    _no_mismatch(big)
    assert np.array_equal(big["steps"], full["steps"])
    assert np.array_equal(_masked(big["binds"], big["steps"], D), fb)
    assert (big["binds"][:, D:] == NONE).all()
    assert np.array_equal(_live(name, big["rows"]), _live(name, full["rows"]))
    # a cap below the behaviours' lengths: their first `cap` steps
    cut = m.selftest_simulate_round(W, cap, seed=seed)
    assert cut["status"] == "ok"
    _no_mismatch(cut)
    want = np.minimum(full["steps"], cap)
    assert np.array_equal(cut["steps"], want)
    assert np.array_equal(_masked(cut["binds"], cut["steps"]), _masked(full["binds"], want, cap))
    res = m.simulate(walkers=W, behaviors=W, depth=cap, seed=seed)
    assert res["status"] == "ok" and res["behaviors"] == W
    assert res["generated"] == W + int(want.sum())
    assert res["depth"] == 1 + int(want.max()) == cap + 1


# ---------------------------------------------------------------- f
def test_capacity_overflow_is_reported():
    name = "raft_n3v1e1r1"
    m, D = _model(name), FIX[name]["depth"]
    assert m.simulate(walkers=4096, depth=D, seed=3, msg_cap_K=1)["status"] == "capacity"
    assert m.selftest_simulate_round(4096, D, seed=3, msg_cap_K=1)["status"] == "capacity"
    assert m.simulate(walkers=4096, depth=D, seed=3)["status"] == "ok"
    assert m.selftest_simulate_round(4096, D, seed=3)["status"] == "ok"
