"""A plain reference for the fingerprint set (raft-tlaplus_amd/csrc/rmc_fpset.h)
and the tools the set's tests share: a dictionary that applies the insert rule,
a builder of keys with a chosen home slot, the scenarios, the decoding of a
dumped table, and a thin wrapper over the test hooks of librmc_selftest.so
(csrc/rmc_selftest_fpset.hip).

The set's contract: no key lost, no key stored twice, the lowest value offered
in a level wins, an earlier level's entry is never touched.  The result of a
batch does not depend on the order of its inserts provided every value stored
by an earlier batch is below the batch's floor, every value of the batch is at
or above it, and the batch's values are distinct; RefSet.apply asserts this on
every batch it is given.
"""
import ctypes
import os

M64 = (1 << 64) - 1
EMPTY = M64
C = 0x9E3779B97F4A7C15          # fp_slot's multiplier (odd: invertible mod 2^64)
C_INV = pow(C, -1, 1 << 64)
assert (C * C_INV) & M64 == 1

# rmc_spec.h ErrCode bits of DevStatus::cap_flags
E_CAP_TABLE, E_RETRY = 8, 10
CAP_TABLE, RETRY = 1 << E_CAP_TABLE, 1 << E_RETRY
# rmc_kernels.hip: candidate ob bits, k_tile_dedup's window, k_insert_recv's records per thread
OB_ERR, OB_LOCAL, OB_TDUP = 0x8000, 0x4000, 0x2000
DEDUP_WIN = 512
RECV_U = 4
PROBE_LIMIT = 4096              # rmc_fpset.h: limit = mask < 4096 ? mask : 4096

GUARD = 16                      # rmc_selftest_fpset.hip: ST_GUARD
DEVICE, RECV = 0, 1             # insert paths of rmc_selftest_fpset_insert


def val_of(rank, hidden):
    """rmc_fpset.h: val = rank << 16 | hidden."""
    assert 0 <= hidden < (1 << 16) and 0 <= rank < (1 << 48)
    return (rank << 16) | hidden


def floor_of(base):
    """rmc_fpset.h: floor = (first global index of the parents' level + 1) << 26;
    `base` is that index + 1, and the level's ranks start at base << 10."""
    return base << 26


def mix64(x):
    """splitmix64's finalizer (a bijection): test data only."""
    z = (x + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def py_fp_slot(fp, slots):
    bits = slots.bit_length() - 1
    return (((fp * C) & M64) >> (64 - bits)) & (slots - 1)


def py_fp_owner(fp, W):
    return ((fp >> 32) * W) >> 32


def key_with_home(slot, slots, salt):
    """The key whose home slot in a table of `slots` entries is `slot`:
    ((slot << sh) | low bits of salt) * C_inv mod 2^64.  Distinct salts below
    2^sh give distinct keys (the low bits are an affine bijection of the salt).
    ~0 (EMPTY) is never returned: the engine maps it away before inserting."""
    assert slots >= 2 and slots & (slots - 1) == 0 and 0 <= slot < slots
    sh = 64 - (slots.bit_length() - 1)
    assert 0 <= salt < (1 << sh) - 1
    low = (salt * 0xD1B54A32D192ED03 + 0x8CB92BA72F3D8DD7) & ((1 << sh) - 1)
    fp = (((slot << sh) | low) * C_INV) & M64
    if fp == EMPTY:  # one key in 2^64: take the reserved last salt's instead
        low = (((1 << sh) - 1) * 0xD1B54A32D192ED03 + 0x8CB92BA72F3D8DD7) & ((1 << sh) - 1)
        fp = (((slot << sh) | low) * C_INV) & M64
    return fp


def second_word(a, salt=0):
    """A second fingerprint word for the 128-bit set (never ~0: a published word)."""
    b = mix64(a ^ (0xA5A5A5A5 + salt))
    return b if b != EMPTY else 0x1234


class RefSet:
    """dict key -> value under the insert rule.  Keys are ints (64-bit set) or
    (a, b) pairs (128-bit set)."""

    def __init__(self):
        self.d = {}

    def copy(self):
        r = RefSet()
        r.d = dict(self.d)
        return r

    def apply(self, keys, vals, floor, continues=False):
        """One batch, in any order.  Returns the set of keys new in this batch.
        continues: the batch is a further chunk of the level the last batch
        began (same floor), as the drivers split a level: stored values at or
        above the floor are then this level's, and the batch's values must
        differ from them too."""
        assert len(keys) == len(vals)
        assert len(set(vals)) == len(vals), "values within a batch are distinct"
        assert all(v >= floor for v in vals), "every batch value is at or above the floor"
        if continues:
            assert not set(vals) & set(self.d.values()), "a level's values are distinct across its chunks"
        else:
            assert all(v < floor for v in self.d.values()), "every earlier value is below the floor"
        assert all(v != EMPTY for v in vals)
        new = set()
        for k, v in zip(keys, vals):
            cur = self.d.get(k)
            if cur is None:
                self.d[k] = v
                new.add(k)
            elif cur >= floor:
                self.d[k] = min(cur, v)
            # else: an earlier level's entry, unchanged
        return new


# ------------------------------------------------------------- dumped tables
def entries(words, ew):
    """The non-empty entries of a dumped table: [(slot, key, val)], key an int
    (ew 2) or (a, b) (ew 4).  Empty slots must be all ~0, and the 128-bit
    entry's unused fourth word stays ~0."""
    out = []
    assert len(words) % ew == 0
    for s in range(len(words) // ew):
        e = words[ew * s: ew * s + ew]
        if e[0] == EMPTY:
            assert all(w == EMPTY for w in e), "slot %d: empty key with words %r" % (s, e)
            continue
        if ew == 2:
            out.append((s, e[0], e[1]))
        else:
            assert e[3] == EMPTY, "slot %d: fourth word written" % s
            out.append((s, (e[0], e[1]), e[2]))
    return out


def check_table(words, ew, ref, probe_reach=None):
    """(a) of the issue: the table's entries, as a multiset of (key, value),
    are exactly the reference's -- none missing, none twice, no value off.
    Also every entry is reachable: no empty slot between its home and its slot
    (what a read-only probe relies on), and, with probe_reach, it lies fewer
    than probe_reach slots from its home.  Returns {key: slot}."""
    slots = len(words) // ew
    ent = entries(words, ew)
    got = sorted((k, v) for _, k, v in ent)
    want = sorted(ref.d.items())
    if got != want:
        gk, wk = dict(got), dict(want)
        dup = len(got) - len(gk)
        missing = [k for k in wk if k not in gk]
        extra = [k for k in gk if k not in wk]
        off = [(k, gk[k], wk[k]) for k in wk if k in gk and gk[k] != wk[k]]
        raise AssertionError("table != reference: %d stored twice, %d missing %r, %d unknown %r, %d values off %r"
                             % (dup, len(missing), missing[:3], len(extra), extra[:3], len(off), off[:3]))
    occupied = [False] * slots
    for s, _, _ in ent:
        occupied[s] = True
    # back[s] = occupied slots in a row ending at s (going round the table's end)
    back = [0] * slots
    run = 0
    for s in list(range(slots)) * 2:
        run = min(run + 1, slots) if occupied[s] else 0
        back[s] = run
    where = {}
    for s, k, _ in ent:
        home = py_fp_slot(k if ew == 2 else k[0], slots)
        dist = (s - home) % slots
        assert back[s] > dist, "key %r at slot %d: empty slot between it and home %d" % (k, s, home)
        if probe_reach is not None:
            assert dist < probe_reach, "key %r lies %d slots from home" % (k, dist)
        where[k] = s
    return where


def check_slots(words, ew, keys, out_slots):
    """(b): every returned slot holds that insert's key; equal keys, equal slots."""
    seen = {}
    for k, s in zip(keys, out_slots):
        assert s != EMPTY, "insert of %r returned no slot" % (k,)
        assert s < len(words) // ew
        got = words[ew * s] if ew == 2 else (words[ew * s], words[ew * s + 1])
        assert got == k, "slot %d holds %r, not the inserted %r" % (s, got, k)
        assert seen.setdefault(k, s) == s
    return seen


def absent_keys(ref, slots, count=48):
    """Keys not in the reference: some with random homes, some whose home is
    the home of a stored key (inside an occupied run), some one slot after."""
    have = set(k if not isinstance(k, tuple) else k[0] for k in ref.d)
    homes = sorted(set(py_fp_slot(a, slots) for a in have))
    out = []
    salt = 1 << 30
    for i in range(count):
        if homes and i % 3 == 0:
            h = homes[(i // 3) % len(homes)]
        elif homes and i % 3 == 1:
            h = (homes[(i // 3) % len(homes)] + 1) % slots
        else:
            h = mix64(i) % slots
        k = key_with_home(h, slots, salt + i)
        assert k not in have
        out.append(k)
    return out


# ------------------------------------------------------------------ scenarios
class Keys:
    """Hands out distinct keys (distinct salts) and distinct ranks."""

    def __init__(self, slots):
        self.slots = slots
        self.salt = 0

    def at(self, home):
        self.salt += 1
        return key_with_home(home % self.slots, self.slots, self.salt)

    def anywhere(self):
        self.salt += 1
        return key_with_home(mix64(self.salt * 977) % self.slots, self.slots, self.salt)


def batch_of(keys, base, hidden=lambda j: (j * 7 + 3) & 0xFFFF):
    """(keys, vals, floor): insert j gets rank (base << 10) + j -- distinct ranks, values at or above the floor."""
    vals = [val_of((base << 10) + j, hidden(j)) for j in range(len(keys))]
    return list(keys), vals, floor_of(base)


def shuffled(keys, seed):
    """A fixed permutation (no RNG state shared between tests)."""
    return [k for _, k in sorted((mix64(seed * 1000003 + i), k) for i, k in enumerate(keys))]


def scn_home_run(slots, home, count):
    """Scenario 1: `count` keys, all with home slot `home`, in one launch (they
    race for the run from an empty table); then, as the next level, up to 9 more
    keys of the same home beside the first ones re-offered -- these find the
    first group already holding other keys and step past it."""
    K = Keys(slots)
    first = [K.at(home) for _ in range(count)]
    more = [K.at(home) for _ in range(min(count, 9))]
    return [batch_of(first, 1), batch_of(shuffled(more + first, 2), 2)]


def scn_interleaved(slots, home, per_home=10):
    """Scenario 2: keys of homes s, s+1, s+2 alternating, each offered twice;
    then, as the next level, as many new keys of the same homes beside the first
    ones re-offered, so a key's first group holds other homes' keys before its own."""
    K = Keys(slots)
    first = [K.at(home + (j % 3)) for j in range(3 * per_home)]
    more = [K.at(home + (j % 3)) for j in range(3 * per_home)]
    return [batch_of(first + first[::-1], 1), batch_of(shuffled(more + first + more, 4), 2)]


def scn_two_chunks(slots, nkeys=60):
    """One level in two launches with the same floor, as the drivers split a
    level into chunks: the second chunk offers the first chunk's keys again, a
    third of them with LOWER values (the stored entry must drop to them: the
    group hit's atomicMin), a third with higher ones (unchanged), beside new
    keys.  An earlier level lies below both."""
    K = Keys(slots)
    old = [K.anywhere() for _ in range(nkeys // 2)]
    ks = [K.anywhere() for _ in range(nkeys)]
    fresh = [K.anywhere() for _ in range(nkeys // 2)]
    base = 4
    c1 = (ks + ks + old[::2], [val_of((base << 10) + 300 + j, (j * 7) & 0xFFFF) for j in range(2 * nkeys + len(old[::2]))],
          floor_of(base))
    lower, higher = ks[0::3], ks[1::3]
    k2 = shuffled(lower + higher + fresh + fresh + old[1::2], 6)
    lowset = set(lower)
    v2 = [val_of((base << 10) + (j if k in lowset else 600 + j), (j * 13 + 1) & 0xFFFF) for j, k in enumerate(k2)]
    return [batch_of(old, 1), c1, (k2, v2, floor_of(base))]


def scn_heavy_dup(slots, arrangement, n=4096, nkeys=37):
    """Scenario 3: n inserts of nkeys keys, all values distinct and differing in
    their low 16 bits.  arrangement: 'adjacent' (a key's duplicates are
    neighbours in a wave), or a distance D (insert j and j + D offer the same key)."""
    K = Keys(slots)
    pool = [K.anywhere() for _ in range(nkeys)]
    if arrangement == "adjacent":
        idx = [j * nkeys // n for j in range(n)]
    else:
        D = int(arrangement)
        assert D >= nkeys and n % D == 0
        idx = [(j % D) * nkeys // D for j in range(n)]
    assert len(set(idx)) == nkeys
    return [batch_of([pool[i] for i in idx], 1, hidden=lambda j: (j * 40503 + 1) & 0xFFFF)]


def scn_three_levels(slots, per_level=40):
    """Scenario 4: three levels with rising floors.  Level 1 (floor 0) holds a
    key with value 0, the initial state.  Levels 2 and 3 re-offer half of every
    earlier level's keys with larger values (those entries must not change) and add
    new keys, each new key offered twice."""
    K = Keys(slots)
    l1 = [K.anywhere() for _ in range(per_level)]
    vals1 = [val_of(0, 0)] + [val_of(1 + j, (j * 5) & 0xFFFF) for j in range(1, per_level)]
    batches = [(l1, vals1, 0)]
    old = list(l1)
    for base in (2, 9):
        fresh = [K.anywhere() for _ in range(per_level)]
        ks = shuffled(old[::2] + fresh + fresh, base)
        batches.append(batch_of(ks, base))
        old += fresh
    return batches


def scn_full(slots):
    """Scenario 5: exactly `slots` distinct keys in one batch, then one more."""
    K = Keys(slots)
    return [batch_of([K.anywhere() for _ in range(slots)], 1)], K.anywhere()


def scn_overflow(slots, count):
    """Scenario 7: more distinct keys than the table has slots (each offered twice)."""
    K = Keys(slots)
    ks = [K.anywhere() for _ in range(count)]
    return batch_of(shuffled(ks + ks, 7), 1)


def widen(batch):
    """The batch with 128-bit keys (a, second_word(a))."""
    keys, vals, floor = batch
    return [(a, second_word(a)) for a in keys], vals, floor


# --------------------------------------------------------------- hook wrappers
def _arr(ctype, seq):
    return (ctype * max(1, len(seq)))(*seq)


_selftest = None


def _lib():
    """The test hooks: librmc_selftest.so, built beside librmc.so (which it links
    against) by `make -C raft-tlaplus_amd`.  Refused when built from other
    sources than the tree's, as raftmc.lib() refuses a stale librmc.so."""
    global _selftest
    if _selftest is not None:
        return _selftest
    import raftmc
    raftmc.lib()
    path = os.path.join(os.path.dirname(raftmc.LIB_PATH), "librmc_selftest.so")
    assert os.path.exists(path), "librmc_selftest.so not built: run `make -C raft-tlaplus_amd` (expected %s)" % path
    L = ctypes.CDLL(path)
    L.rmc_selftest_source_id.restype = ctypes.c_char_p
    stale = raftmc.source_mismatch(L.rmc_selftest_source_id().decode())
    assert stale is None or os.environ.get("RAFTMC_ALLOW_STALE") == "1", "%s is stale (%s): rebuild it" % (path, stale)
    P, c_int, u64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_uint64
    U64P, U32P, U8P = (ctypes.POINTER(t) for t in (ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint8))
    L.rmc_selftest_fp_slot.argtypes = [u64, u64]
    L.rmc_selftest_fp_slot.restype = u64
    L.rmc_selftest_fp_owner.argtypes = [u64, c_int]
    L.rmc_selftest_fpset_new.argtypes = [c_int, u64]
    L.rmc_selftest_fpset_new.restype = P
    L.rmc_selftest_fpset_free.argtypes = [P]
    L.rmc_selftest_fpset_free.restype = None
    L.rmc_selftest_fpset_slots.argtypes = [P]
    L.rmc_selftest_fpset_slots.restype = ctypes.c_int64
    L.rmc_selftest_fpset_insert.argtypes = [P, c_int, U64P, U64P, u64, u64, U64P, U32P, U64P]
    L.rmc_selftest_fpset_lookup.argtypes = [P, U64P, u64, U64P]
    L.rmc_selftest_fpset_grow.argtypes = [P, u64, U32P]
    L.rmc_selftest_fpset_reset_ranks.argtypes = [P, u64, u64]
    L.rmc_selftest_fpset_mark_recv.argtypes = [P, u64, u64, U8P, U64P, U64P]
    L.rmc_selftest_fpset_dump.argtypes = [P, U64P, u64]
    L.rmc_selftest_fpset_dump.restype = ctypes.c_int64
    L.rmc_selftest_owner_partition.argtypes = [U64P, U64P, U32P, u64, c_int, U64P, U32P, U32P]
    L.rmc_selftest_tile_dedup.argtypes = [U32P, U32P, u64, U64P, U64P, U32P, u64]
    # the hooks report through librmc's rmc_last_error
    L.rmc_last_error = raftmc.lib().rmc_last_error
    _selftest = L
    return L


def _err():
    return _lib().rmc_last_error().decode()


def hook_fp_slot(fp, slots):
    return _lib().rmc_selftest_fp_slot(fp, slots - 1)


def hook_fp_owner(fp, W):
    return _lib().rmc_selftest_fp_owner(fp, W)


def verify_homes(keys, slots):
    """Every built key's home through the fp_slot hook: the Python arithmetic
    that chose it is never trusted."""
    for k in keys:
        a = k[0] if isinstance(k, tuple) else k
        assert a != EMPTY
        assert hook_fp_slot(a, slots) == py_fp_slot(a, slots), hex(a)


class DeviceSet:
    """The fingerprint set on the GPU through rmc_selftest_fpset_*."""

    def __init__(self, fp_bits, slots):
        self.L = _lib()
        self.ew = 4 if fp_bits == 128 else 2
        self.h = self.L.rmc_selftest_fpset_new(fp_bits, slots)
        assert self.h, _err()

    @property
    def slots(self):
        return self.L.rmc_selftest_fpset_slots(self.h)

    def close(self):
        if self.h:
            self.L.rmc_selftest_fpset_free(self.h)
        self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def insert(self, path, keys, vals, floor):
        """-> (slots, cap_flags).  self.raw = k_insert_recv's slot words (recv path)."""
        n = len(keys)
        flat = [w for k in keys for w in k] if self.ew == 4 else keys
        out, raw, flags = _arr(ctypes.c_uint64, [0] * n), _arr(ctypes.c_uint64, [0] * n), ctypes.c_uint32(0xFFFFFFFF)
        rc = self.L.rmc_selftest_fpset_insert(self.h, path, _arr(ctypes.c_uint64, flat), _arr(ctypes.c_uint64, vals), n,
                                              floor, out, ctypes.byref(flags), raw)
        assert rc == 0, _err()
        self.raw = list(raw[:n])
        return list(out[:n]), flags.value

    def lookup(self, keys):
        n = len(keys)
        out = _arr(ctypes.c_uint64, [0] * n)
        rc = self.L.rmc_selftest_fpset_lookup(self.h, _arr(ctypes.c_uint64, keys), n, out)
        assert rc == 0, _err()
        return list(out[:n])

    def grow(self, new_slots):
        flags = ctypes.c_uint32(0xFFFFFFFF)
        rc = self.L.rmc_selftest_fpset_grow(self.h, new_slots, ctypes.byref(flags))
        assert rc == 0, _err()
        return flags.value

    def reset_ranks(self, lo, hi):
        rc = self.L.rmc_selftest_fpset_reset_ranks(self.h, lo, hi)
        assert rc == 0, _err()

    def mark_recv(self, n, floor):
        """-> (flags, newcount, hidden_coll) for the last recv-path batch."""
        fl = _arr(ctypes.c_uint8, [0] * n)
        nc, hc = ctypes.c_uint64(M64), ctypes.c_uint64(M64)
        rc = self.L.rmc_selftest_fpset_mark_recv(self.h, n, floor, fl, ctypes.byref(nc), ctypes.byref(hc))
        assert rc == 0, _err()
        return list(fl[:n]), nc.value, hc.value

    def dump(self):
        """The table's words.  The hook's table has GUARD more entries behind the
        last slot, outside the set: they must still be ~0 (a probe that stepped
        past the end without wrapping would have written there)."""
        n = self.slots * self.ew
        cap = n + GUARD * self.ew
        out = (ctypes.c_uint64 * cap)()
        got = self.L.rmc_selftest_fpset_dump(self.h, out, cap)
        assert got == cap, _err()
        assert all(w == EMPTY for w in out[n:]), "written past the last slot: %r" % [hex(w) for w in out[n:n + 8]]
        return list(out[:n])


def plain_lookup(words, ew, key):
    """A read-only probe of a dumped table, as fpset_value walks it: the value
    of `key`, ~0 when an empty slot ends the run (or the whole table was walked)."""
    slots = len(words) // ew
    s = py_fp_slot(key if ew == 2 else key[0], slots)
    for _ in range(slots):
        e = words[ew * s: ew * s + ew]
        if e[0] == EMPTY:
            return EMPTY
        if (ew == 2 and e[0] == key) or (ew == 4 and (e[0], e[1]) == key):
            return e[ew >> 1]
        s = (s + 1) % slots
    return EMPTY


def run_batch(S, path, batch, ref, expect_flags=0, probe_reach=None, continues=False):
    """Insert one batch into set S and assert (a)-(d) of the issue against the
    reference, which is advanced by the batch.  Returns (slots, new keys)."""
    keys, vals, floor = batch
    verify_homes(keys, S.slots)
    new = ref.apply(keys, vals, floor, continues)
    got, flags = S.insert(path, keys, vals, floor)
    if S.ew == 4 and flags == expect_flags | RETRY:
        # fp_bits 128: a lane may find a key claimed and its second word not yet
        # published (E_RETRY).  Every key of the batch is complete by now, so ONE
        # redo of the same batch must come back without it.
        got, flags = S.insert(path, keys, vals, floor)
    assert flags == expect_flags, "cap_flags %#x" % flags                  # (d)
    if path == RECV:  # k_insert_recv's slot words: hidden << 47 | slot
        assert S.raw == [((v & 0xFFFF) << 47) | s for v, s in zip(vals, got)]
    words = S.dump()
    check_table(words, S.ew, ref, probe_reach)                              # (a)
    check_slots(words, S.ew, keys, got)                                     # (b)
    check_lookups(S, words, ref)                                            # (c)
    return got, new


def check_lookups(S, words, ref):
    """(c): every stored key reads back its reference value and absent keys
    read ~0 -- through fpset_value on the device (64-bit set), and through a
    plain probe of the dump (every set)."""
    slots = len(words) // S.ew
    present = list(ref.d)
    absent = absent_keys(ref, slots)
    if S.ew == 4:
        # absent 128-bit keys: unknown first words, and a STORED first word with another second word
        absent = [(a, second_word(a)) for a in absent] + [(k[0], k[1] ^ 1) for k in present[:16]]
    # (a long run makes the plain probe quadratic: a spread sample of it then; check_table covered every key)
    for k in present if len(present) <= 512 else present[::len(present) // 128] + present[-8:]:
        assert plain_lookup(words, S.ew, k) == ref.d[k]
    for k in absent:
        assert k not in ref.d and plain_lookup(words, S.ew, k) == EMPTY
    if S.ew == 2:
        assert S.lookup(present) == [ref.d[k] for k in present]
        assert S.lookup(absent) == [EMPTY] * len(absent)
