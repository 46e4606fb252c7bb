"""The fingerprint-set kernels against a plain reference set.

The production code -- fpset_insert / fpset_insert128 / fpset_value
(rmc_fpset.h), k_insert_recv, k_mark_recv, k_rehash, k_reset_ranks,
k_owner_count + k_bucket and k_tile_dedup (rmc_kernels.hip) -- runs through
the hooks of rmc_selftest_fpset.hip on small tables whose keys are built to
land in chosen home slots, and every result is compared with a dictionary
(tests/fpset_ref.py).  After each insert batch: (a) the dumped table equals the
reference as a multiset of (key, value); (b) every returned slot holds its key,
equal keys got equal slots; (c) every key reads back its value and absent keys
read ~0; (d) no status flag unless the scenario says so.

Paths: p64 = a thread per key calls fpset_insert, recv = launch_insert_recv on
(fp, val) records, p128 = a thread per key calls fpset_insert128.
"""
import ctypes

import pytest

import fpset_ref as R
from fpset_ref import CAP_TABLE, DEVICE, EMPTY, OB_ERR, OB_LOCAL, OB_TDUP, RECV, RETRY, RefSet

pytestmark = pytest.mark.gpu

PATHS = {"p64": (64, DEVICE), "recv": (64, RECV), "p128": (128, DEVICE)}
ALL = list(PATHS)


def open_set(path, slots):
    return R.DeviceSet(PATHS[path][0], slots)


def adapt(path, batch):
    return R.widen(batch) if PATHS[path][0] == 128 else batch


def run(S, path, batch, ref, **kw):
    return R.run_batch(S, PATHS[path][1], adapt(path, batch), ref, **kw)


def insert_with_one_redo(S, path, batch, allowed):
    """An insert whose flags may hold E_RETRY once (fp_bits 128): one redo of the
    same batch must then come back without it."""
    keys, vals, floor = batch
    got, flags = S.insert(PATHS[path][1], keys, vals, floor)
    if S.ew == 4 and flags & RETRY:
        got, flags = S.insert(PATHS[path][1], keys, vals, floor)
    assert flags in allowed, "cap_flags %#x" % flags
    return got, flags


# ----------------------------------------------------- 1. home slot placement
@pytest.mark.parametrize("path", ALL)
@pytest.mark.parametrize("count", [1, 4, 5, 9, 200])
@pytest.mark.parametrize("home", ["mid", -4, -3, -2, -1, 0])
def test_home_slot_placement(home, count, path):
    """All keys of a batch share one home slot: a middle slot, slots-4 (the last
    home whose group load is taken), slots-3 and slots-1 (group skipped), slots-2
    (the last home of the 128-bit fast path), 0.  A
    second batch of the same home finds the group full of other keys (at slots-4
    the step past it must wrap to slot 0).  The run crosses the last slot and
    wraps; it is one gapless run from the home."""
    slots = 256
    h = 117 if home == "mid" else home % slots
    ref = RefSet()
    with open_set(path, slots) as S:
        for b in R.scn_home_run(slots, h, count):
            run(S, path, b, ref)
        assert sorted(s for s, _, _ in R.entries(S.dump(), S.ew)) == sorted((h + q) % slots for q in range(count + min(count, 9)))


# --------------------------------------------------------- 2. interleaved runs
@pytest.mark.parametrize("path", ALL)
@pytest.mark.parametrize("home", [100, 252, 254])
def test_interleaved_runs(home, path):
    """Homes s, s+1, s+2 alternating: the first group holds other keys before a key's own."""
    ref = RefSet()
    with open_set(path, 256) as S:
        for b in R.scn_interleaved(256, home):
            run(S, path, b, ref)


# -------------------------------------------------------- 3. heavy duplication
@pytest.mark.parametrize("path", ALL)
@pytest.mark.parametrize("arrangement", ["adjacent", 64, 256 * R.RECV_U])
def test_heavy_duplication(arrangement, path):
    """4096 inserts of 37 keys with distinct values (low 16 bits differ): every
    key ends at the minimum offered, whichever lane claimed it."""
    ref = RefSet()
    with open_set(path, 256) as S:
        for b in R.scn_heavy_dup(256, arrangement):
            run(S, path, b, ref)
        assert len(ref.d) == 37


# --------------------------------------------------------------- 4. three levels
@pytest.mark.parametrize("path", ALL)
def test_three_levels(path):
    """Rising floors; a value 0 in level 1; re-offered keys of earlier levels stay bit-identical."""
    ref = RefSet()
    with open_set(path, 256) as S:
        for b in R.scn_three_levels(256):
            before = {k: v for _, k, v in R.entries(S.dump(), S.ew)}
            run(S, path, b, ref)
            after = {k: v for _, k, v in R.entries(S.dump(), S.ew)}
            assert all(after[k] == v for k, v in before.items())
        assert 0 in ref.d.values()


@pytest.mark.parametrize("path", ALL)
def test_level_in_two_chunks(path):
    """A level inserted in two launches with one floor: an entry of the first
    chunk drops to a lower value of the second (a group hit's atomicMin), keeps
    its own against a higher one, and the earlier level's entries stay."""
    ref = RefSet()
    with open_set(path, 256) as S:
        b0, c1, c2 = R.scn_two_chunks(256)
        run(S, path, b0, ref)
        run(S, path, c1, ref)
        mid = dict(ref.d)
        run(S, path, c2, ref, continues=True)
        key = (lambda a: (a, R.second_word(a))) if S.ew == 4 else (lambda a: a)
        assert sum(ref.d[k] < v for k, v in mid.items()) == 20   # exactly the re-offered third dropped
        assert all(ref.d[key(a)] == mid[key(a)] for a in b0[0])


# ------------------------------------------------------------ 5. small full table
@pytest.mark.parametrize("path", ALL)
def test_small_full_table(path):
    """64 slots, 64 distinct keys in one launch: all stored, no flag (the probe
    loop covers every slot when mask < 4096).  One more key: EMPTY, E_CAP_TABLE,
    table unchanged."""
    ref = RefSet()
    batches, extra = R.scn_full(64)
    with open_set(path, 64) as S:
        run(S, path, batches[0], ref)
        before = S.dump()
        more = adapt(path, ([extra], [R.val_of(5 << 10, 1)], R.floor_of(5)))
        got, flags = insert_with_one_redo(S, path, more, {CAP_TABLE})
        assert got == [EMPTY]
        assert S.dump() == before


@pytest.mark.parametrize("path", ALL)
def test_last_free_slot_before_home(path):
    """The probe loop's last step: 63 keys sit in their home slots, every slot
    but 62; a key whose home is the LAST slot (no group load, no fast path) must
    walk all 64 slots and take slot 62 -- probe index 63 = the limit itself."""
    slots = 64
    ref = RefSet()
    with open_set(path, slots) as S:
        first = R.batch_of([R.key_with_home(q, slots, 100 + q) for q in range(slots) if q != 62], 1)
        run(S, path, first, ref)
        last = R.batch_of([R.key_with_home(63, slots, 999)], 3)
        got, _ = run(S, path, last, ref)
        assert got == [62]


# ------------------------------------------------------------------ 6. probe limit
# the farthest slot an insert can claim, in slots from the key's home: the group
# (4 entries; 2 on fp_bits 128) plus the CAS loop's probes 0..4096
MAX_DIST = {"p64": 4 + R.PROBE_LIMIT, "recv": 4 + R.PROBE_LIMIT, "p128": 2 + R.PROBE_LIMIT}


@pytest.mark.parametrize("path", ALL)
def test_probe_limit_not_reached(path):
    """8192 slots, one home, a run of 4097 keys: no flag, and no key more than 4096 slots from home."""
    slots, home = 8192, 6000  # the run wraps past the last slot
    ref = RefSet()
    with open_set(path, slots) as S:
        run(S, path, R.scn_home_run(slots, home, R.PROBE_LIMIT + 1)[0], ref, probe_reach=R.PROBE_LIMIT + 1)


@pytest.mark.parametrize("path", ALL)
def test_probe_limit_exceeded(path):
    """A run of 4102 keys is longer than any insert can reach: E_CAP_TABLE, at
    least one insert returns EMPTY, and every insert that returned a slot is
    stored with its value (the documented capacity flag only)."""
    slots, home, count = 8192, 6000, 4102
    batch = adapt(path, R.scn_home_run(slots, home, count)[0])
    keys, vals, floor = batch
    R.verify_homes(keys, slots)
    with open_set(path, slots) as S:
        got, flags = insert_with_one_redo(S, path, batch, {CAP_TABLE})
        failed = [j for j, s in enumerate(got) if s == EMPTY]
        assert len(failed) >= count - (MAX_DIST[path] + 1) >= 1
        ok = [j for j, s in enumerate(got) if s != EMPTY]
        ref = RefSet()
        ref.apply([keys[j] for j in ok], [vals[j] for j in ok], floor)
        words = S.dump()
        R.check_table(words, S.ew, ref, probe_reach=MAX_DIST[path] + 1)
        R.check_slots(words, S.ew, [keys[j] for j in ok], [got[j] for j in ok])


# ------------------------------------------------------- 7. overflow, grow, redo
@pytest.mark.parametrize("path", ALL)
@pytest.mark.parametrize("factor", [2, 8])
def test_overflow_grow_redo(factor, path):
    """A batch overflows a 64-slot table; launch_rehash into 2x / 8x keeps every
    entry (key, second word, value); the same batch again gives the reference:
    the driver's recovery contract."""
    slots = 64
    with open_set(path, slots) as S:
        ref = RefSet()
        run(S, path, R.batch_of([R.key_with_home(q, slots, 5000 + q) for q in range(0, 64, 4)], 0), ref)
        settled = dict(ref.d)
        batch = adapt(path, R.scn_overflow(slots, 100))
        keys, vals, floor = batch
        got, flags = insert_with_one_redo(S, path, batch, {CAP_TABLE})
        assert EMPTY in got
        partial = {k: v for _, k, v in R.entries(S.dump(), S.ew)}
        assert len(partial) == slots and all(partial[k] == v for k, v in settled.items())
        assert S.grow(slots * factor) == 0
        grown = RefSet()
        grown.d = partial
        words = S.dump()
        R.check_table(words, S.ew, grown)      # grow alone: every entry kept, each reachable from its new home
        R.check_lookups(S, words, grown)
        ref.apply(keys, vals, floor)
        got, flags = insert_with_one_redo(S, path, batch, {0})
        words = S.dump()
        R.check_table(words, S.ew, ref)
        R.check_slots(words, S.ew, keys, got)
        R.check_lookups(S, words, ref)


# ------------------------------------------------- 8. n edge cases, recv path
@pytest.mark.parametrize("n", [0, 1, 255, 1023, 1024, 1025])
def test_recv_batch_sizes(n):
    """n around 256 x RECV_U records per block: every record gets its slot word, none past n is touched."""
    slots = 4096
    K = R.Keys(slots)
    pool = [K.anywhere() for _ in range(n // 2 + 1)]
    ref = RefSet()
    with open_set("recv", slots) as S:
        run(S, "recv", R.batch_of([pool[(j * 5) % len(pool)] for j in range(n)], 1), ref)
        if n == 0:
            assert R.entries(S.dump(), 2) == []


# -------------------------------------------------------------- 9. 128-bit only
def _same_first_word_groups(slots):
    """Groups of 2, 3 and 8 keys with equal first words and different second
    words, and pairs with equal second words and different first words."""
    K = R.Keys(slots)
    groups = []
    for size, home in ((2, 10), (3, 11), (8, slots - 1), (2, slots - 2), (3, 40)):
        a = K.at(home)
        groups.append([(a, R.second_word(a, i)) for i in range(size)])
    b = 0x1122334455667788
    same_b = [(K.at(41), b), (K.at(41), b), (K.anywhere(), b)]
    return groups, same_b


@pytest.mark.parametrize("split", ["one_batch", "across_batches"])
def test_fp128_equal_first_words(split):
    """Keys that differ only in the second word are distinct entries, whether
    they meet in one launch (claim / publish race; E_RETRY is legal once) or
    the first word is found already stored."""
    slots = 256
    groups, same_b = _same_first_word_groups(slots)
    flat = [k for g in groups for k in g] + same_b
    assert len(set(flat)) == len(flat)
    ref = RefSet()
    with open_set("p128", slots) as S:
        if split == "one_batch":
            keys = R.shuffled(flat + flat, 3)
            R.run_batch(S, DEVICE, R.batch_of(keys, 1), ref)
        else:
            firsts = [g[0] for g in groups] + same_b[:1]
            rest = [k for g in groups for k in g[1:]] + same_b[1:]
            R.run_batch(S, DEVICE, R.batch_of(firsts, 1), ref)
            # the second batch re-offers the stored keys too (they must not change)
            R.run_batch(S, DEVICE, R.batch_of(R.shuffled(rest + rest + firsts, 5), 2), ref)
        assert len(ref.d) == len(flat)
        assert len(R.entries(S.dump(), 4)) == len(flat)


# ------------------------------------------------------------- 10. reset_ranks
@pytest.mark.parametrize("path", ALL)
def test_reset_ranks(path):
    """Ranks on both sides of [lo, hi), entries exactly at lo, hi-1 and hi, and a
    value 0: exactly the in-range values become ~0, keys and empty slots are
    untouched; re-inserting the range's keys then matches the reference."""
    slots = 256
    lo, hi = 5 << 10, 7 << 10
    ranks = [0, 1, lo - 2, lo - 1, lo, lo + 1, lo + 700, hi - 2, hi - 1, hi, hi + 1, hi + 900, 9 << 10]
    K = R.Keys(slots)
    keys = [K.anywhere() for _ in ranks] + [K.at(slots - 2) for _ in range(3)]
    ranks = ranks + [lo + 3, hi + 3, lo + 4]
    vals = [R.val_of(r, (i * 11) & 0xFFFF if r else 0) for i, r in enumerate(ranks)]
    keys, vals, _ = adapt(path, (keys, vals, 0))
    ref = RefSet()
    with open_set(path, slots) as S:
        R.run_batch(S, PATHS[path][1], (keys, vals, 0), ref)
        before = S.dump()
        S.reset_ranks(lo, hi)
        after = S.dump()
        ew, vw = S.ew, S.ew >> 1
        in_range = set()
        for s in range(slots):
            e0, e1 = before[ew * s: ew * s + ew], after[ew * s: ew * s + ew]
            hit = e0[0] != EMPTY and lo <= (e0[vw] >> 16) < hi
            want = list(e0)
            if hit:
                want[vw] = EMPTY
                in_range.add(e0[0] if ew == 2 else (e0[0], e0[1]))
            assert e1 == want, "slot %d: %r -> %r" % (s, e0, e1)
        assert in_range == {k for k, r in zip(keys, ranks) if lo <= r < hi} and len(in_range) == 7
        # the redo: the range's keys offered again (twice each) with new values of the same range
        again = R.shuffled(sorted(in_range) * 2, 9)
        floor = lo << 16
        nvals = [R.val_of(lo + 20 + j, (j * 3) & 0xFFFF) for j in range(len(again))]
        later = {k: v for k, v in ref.d.items() if v >= floor and k not in in_range}
        for k in list(in_range) + list(later):
            del ref.d[k]
        ref.apply(again, nvals, floor)   # (entries of later ranks hold other keys: set aside for the precondition)
        ref.d.update(later)
        got, flags = insert_with_one_redo(S, path, (again, nvals, floor), {0})
        words = S.dump()
        R.check_table(words, ew, ref)
        R.check_slots(words, ew, again, got)
        R.check_lookups(S, words, ref)


# --------------------------------------------------------------- 11. mark_recv
def test_mark_recv():
    """After a recv batch: flag 1 exactly for the record holding a new key's
    minimum value, 2 exactly for same-batch losers whose low 16 bits differ from
    the winner's, 0 otherwise (duplicates of an earlier batch's key included);
    newcount = new keys, hidden_coll = flag-2 records."""
    slots = 2048
    K = R.Keys(slots)
    old = [K.anywhere() for _ in range(300)]
    fresh = [K.anywhere() for _ in range(400)]
    ref = RefSet()
    with open_set("recv", slots) as S:
        b1 = R.batch_of(old, 0)
        R.run_batch(S, RECV, b1, ref)
        fl, nc, hc = S.mark_recv(len(old), b1[2])
        assert fl == [1] * len(old) and nc == len(old) and hc == 0
        # batch 2: 1500 records -- each fresh key 2 or 3 times, hidden bits from {0, 1}
        # (so losers both with and without a collision), and old keys again
        keys = [fresh[j % 400] for j in range(1100)] + [old[j % 300] for j in range(400)]
        keys = R.shuffled(keys, 11)
        b2 = R.batch_of(keys, 3, hidden=lambda j: (j >> 2) & 1)
        _, vals, floor = b2
        _, new = R.run_batch(S, RECV, b2, ref)
        assert new == set(fresh)
        fl, nc, hc = S.mark_recv(len(keys), floor)
        want = []
        for k, v in zip(keys, vals):
            if k not in new:
                want.append(0)
            elif ref.d[k] == v:
                want.append(1)
            else:
                want.append(2 if (ref.d[k] ^ v) & 0xFFFF else 0)
        assert fl == want
        assert want.count(2) > 50 and want.count(0) > 450  # the scenario has both kinds of loser
        assert nc == len(new) == want.count(1)
        assert hc == want.count(2)


# ----------------------------------------------------------- 12. owner partition
def _partition(L, fp, val, ob, W):
    n = len(fp)
    send, perm, cnt = (ctypes.c_uint64 * (2 * n))(), (ctypes.c_uint32 * n)(), (ctypes.c_uint32 * W)()
    rc = L.rmc_selftest_owner_partition(R._arr(ctypes.c_uint64, fp), R._arr(ctypes.c_uint64, val),
                                        R._arr(ctypes.c_uint32, ob), n, W, send, perm, cnt)
    assert rc == 0, L.rmc_last_error()
    return list(send), list(perm), list(cnt)


@pytest.mark.parametrize("W", [1, 2, 3, 8, 64])
@pytest.mark.parametrize("n", [1, 255, 256, 257, 5000])
def test_owner_partition(n, W):
    """k_owner_count + scan + k_bucket: owner o's segment of the send buffer is
    exactly the multiset of remote candidates with fp_owner = o; perm[t] points at
    candidate t's record; excluded candidates (OB_ERR / OB_LOCAL / OB_TDUP) get
    0xFFFFFFFF; the counts sum to the number of remote candidates."""
    L = R._lib()
    fp, val, ob = [], [], []
    for t in range(n):
        f = R.mix64(t * 31 + n)
        if t % 7 == 0:
            f &= 0xFFFFFFFF                      # high word 0x00000000: owner 0
        elif t % 7 == 1:
            f |= 0xFFFFFFFF00000000              # high word 0xFFFFFFFF: owner W-1
        fp.append(f)
        val.append(R.val_of((1 << 10) + t, t & 0xFFFF))
        o = ((t % 13) << 16) | (t % 50)
        if n > 1:
            o |= {0: OB_ERR, 3: OB_LOCAL, 5: OB_TDUP, 8: OB_ERR | OB_TDUP}.get(t % 11, 0)
        ob.append(o)
    send, perm, cnt = _partition(L, fp, val, ob, W)
    remote = [t for t in range(n) if not ob[t] & (OB_ERR | OB_LOCAL | OB_TDUP)]
    owners = {t: R.py_fp_owner(fp[t], W) for t in remote}
    for t in remote:
        assert R.hook_fp_owner(fp[t], W) == owners[t]
        if fp[t] >> 32 == 0:
            assert owners[t] == 0
        if fp[t] >> 32 == 0xFFFFFFFF:
            assert owners[t] == W - 1
    assert sum(cnt) == len(remote)
    assert cnt == [sum(1 for t in remote if owners[t] == o) for o in range(W)]
    start = 0
    for o in range(W):
        seg = sorted((send[2 * p], send[2 * p + 1]) for p in range(start, start + cnt[o]))
        assert seg == sorted((fp[t], val[t]) for t in remote if owners[t] == o)
        start += cnt[o]
    assert all(w == EMPTY for w in send[2 * start:])          # nothing behind the last segment
    for t in range(n):
        if t in owners:
            assert perm[t] < len(remote) and (send[2 * perm[t]], send[2 * perm[t] + 1]) == (fp[t], val[t])
        else:
            assert perm[t] == 0xFFFFFFFF
    assert len(set(perm[t] for t in remote)) == len(remote)


# ---------------------------------------------------------------- 13. tile dedup
def _dedup_reference(par_off, par_n, fp, val, ob):
    """k_tile_dedup's rule, plainly: per tile of 64 parents, per window of
    DEDUP_WIN candidates, among the candidates that are neither OB_ERR nor
    OB_LOCAL: the minimum-value candidate of a key is its representative; another
    candidate of that key whose hidden bits equal the representative's becomes
    OB_TDUP with cand_val = the representative's index; all else is unchanged."""
    val, ob = list(val), list(ob)
    npar = len(par_off)
    for p0 in range(0, npar, 64):
        pl = min(npar, p0 + 64) - 1
        t0, t1 = par_off[p0], par_off[pl] + par_n[pl]
        for w0 in range(t0, t1, R.DEDUP_WIN):
            idx = [t for t in range(w0, min(t1, w0 + R.DEDUP_WIN)) if not ob[t] & (OB_ERR | OB_LOCAL)]
            rep = {}
            for t in idx:
                if fp[t] not in rep or val[t] < val[rep[fp[t]]]:
                    rep[fp[t]] = t
            snapshot = {t: val[t] for t in idx}
            for t in idx:
                r = rep[fp[t]]
                if t != r and (snapshot[t] ^ snapshot[r]) & 0xFFFF == 0:
                    ob[t] |= OB_TDUP
                    val[t] = r
    return val, ob


@pytest.mark.parametrize("nparents", [64, 130, 192])
@pytest.mark.parametrize("per_parent", [3, 20])
def test_tile_dedup(per_parent, nparents):
    """One tile, three tiles and a short last tile; tile ranges shorter
    (3 x 64 = 192) and longer (20 x 64 = 1280) than DEDUP_WIN = 512.  An OB_TDUP
    candidate is never the minimum of its key in its window, its cand_val is the
    index of that minimum, its hidden bits equal the representative's; repeats
    with other hidden bits, repeats across windows and tiles, and OB_ERR /
    OB_LOCAL candidates are unchanged."""
    L = R._lib()
    par_n = [per_parent + (p % 3 == 0) - (p % 5 == 0) for p in range(nparents)]
    par_off = [sum(par_n[:p]) for p in range(nparents)]
    n = sum(par_n)
    fp, val, ob = [], [], []
    t = 0
    for p in range(nparents):
        for o in range(par_n[p]):
            # ~150 keys per tile (repeats inside a window and across windows), some shared between tiles
            tile = p // 64
            fp.append(R.mix64((tile if t % 9 else 0) * 1000 + R.mix64(t) % 150))
            val.append(R.val_of(((p + 1) << 10) | o, R.mix64(t * 3) % 3))
            flags = {4: OB_ERR, 9: OB_LOCAL}.get(t % 17, 0)
            ob.append((o << 16) | (t % 40) | flags)
            t += 1
    assert len(set(val)) == n
    want_val, want_ob = _dedup_reference(par_off, par_n, fp, val, ob)
    cval, cob = R._arr(ctypes.c_uint64, val), R._arr(ctypes.c_uint32, ob)
    rc = L.rmc_selftest_tile_dedup(R._arr(ctypes.c_uint32, par_off), R._arr(ctypes.c_uint32, par_n), nparents,
                                   R._arr(ctypes.c_uint64, fp), cval, cob, n)
    assert rc == 0, L.rmc_last_error()
    got_val, got_ob = list(cval[:n]), list(cob[:n])
    tdup = [t for t in range(n) if got_ob[t] & OB_TDUP]
    for t in tdup:
        r = got_val[t]
        assert r < n and fp[r] == fp[t] and val[r] < val[t] and not got_ob[r] & OB_TDUP
        assert (val[r] ^ val[t]) & 0xFFFF == 0
        assert not ob[t] & (OB_ERR | OB_LOCAL)
    assert got_ob == want_ob and got_val == want_val
    # the scenario has what it claims: dedups, same-window repeats with other hidden bits left alone
    assert len(tdup) > n // 20
    assert any(not got_ob[t] & OB_TDUP and got_val[t] == val[t] and fp[t] in set(fp[:t]) for t in range(n))


# ------------------------------------------------------------ argument checks
def test_hooks_refuse_bad_arguments():
    """A bad argument never reaches a kernel: negative return, rmc_last_error set."""
    L = R._lib()
    u64 = (ctypes.c_uint64 * 8)()
    u32 = (ctypes.c_uint32 * 8)()
    with R.DeviceSet(64, 64) as S, R.DeviceSet(128, 64) as S128:
        fl = ctypes.c_uint32()
        assert L.rmc_selftest_fpset_insert(S.h, 2, u64, u64, 1, 0, u64, ctypes.byref(fl), None) < 0
        assert L.rmc_selftest_fpset_insert(S128.h, RECV, u64, u64, 1, 0, u64, ctypes.byref(fl), None) < 0
        assert L.rmc_selftest_fpset_insert(S.h, 0, u64, u64, 1 << 40, 0, u64, ctypes.byref(fl), None) < 0
        assert L.rmc_selftest_fpset_insert(S.h, 0, None, u64, 1, 0, u64, ctypes.byref(fl), None) < 0
        assert L.rmc_selftest_fpset_lookup(S128.h, u64, 1, u64) < 0
        assert L.rmc_selftest_fpset_grow(S.h, 64, ctypes.byref(fl)) < 0
        assert L.rmc_selftest_fpset_grow(S.h, 96, ctypes.byref(fl)) < 0
        assert L.rmc_selftest_fpset_reset_ranks(S.h, 5, 4) < 0
        assert L.rmc_selftest_fpset_mark_recv(S.h, 1, 0, ctypes.cast(u64, ctypes.POINTER(ctypes.c_uint8)), u64, u64) < 0
        assert L.rmc_selftest_fpset_dump(S.h, u64, 8) < 0
        assert b"rmc_selftest_fpset" in L.rmc_last_error()
        assert R.entries(S.dump(), 2) == [] and R.entries(S128.dump(), 4) == []
    assert L.rmc_selftest_owner_partition(u64, u64, u32, 0, 2, u64, u32, u32) < 0
    assert L.rmc_selftest_owner_partition(u64, u64, u32, 1, 65, u64, u32, u32) < 0
    off, cnt = (ctypes.c_uint32 * 2)(0, 5), (ctypes.c_uint32 * 2)(4, 4)   # a gap, and past ncand
    assert L.rmc_selftest_tile_dedup(off, cnt, 2, u64, u64, u32, 8) < 0
    off = (ctypes.c_uint32 * 2)(0, 4)
    assert L.rmc_selftest_tile_dedup(off, cnt, 2, u64, u64, u32, 7) < 0
