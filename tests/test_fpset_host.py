"""The fingerprint-set harness without a GPU: the key builder and the slot /
owner functions through the test library's host-only hooks, the reference's
rule and preconditions, the scenarios the builders emit, and the hooks'
argument checks that need no device.  The scenarios themselves run on the HIP
kernels in test_gpu_fpset.py."""
import ctypes

import pytest

import fpset_ref as R
from fpset_ref import EMPTY, RefSet


# ------------------------------------------------------------ builder, hooks
@pytest.mark.parametrize("slots", [8, 64, 256, 8192, 1 << 20])
def test_key_builder_homes(slots):
    """key_with_home lands where asked, by the library's fp_slot; keys are distinct and never ~0."""
    seen = set()
    homes = sorted({0, 1, slots // 2, slots - 4, slots - 3, slots - 1})
    for h in homes:
        for salt in range(40):
            k = R.key_with_home(h, slots, salt * len(homes) + homes.index(h))
            assert k != EMPTY and k not in seen
            seen.add(k)
            assert R.hook_fp_slot(k, slots) == h
            assert R.py_fp_slot(k, slots) == h


def test_fp_slot_matches_python_on_mixed_keys():
    for slots in (8, 256, 1 << 30):
        for i in range(500):
            fp = R.mix64(i)
            assert R.hook_fp_slot(fp, slots) == R.py_fp_slot(fp, slots)


def test_fp_owner_hook():
    for W in (1, 2, 3, 8, 64):
        assert R.hook_fp_owner(0x00000000FFFFFFFF, W) == 0
        assert R.hook_fp_owner(0xFFFFFFFF00000000, W) == W - 1
        prev = 0
        for i in range(400):
            fp = R.mix64(i)
            o = R.hook_fp_owner(fp, W)
            assert o == R.py_fp_owner(fp, W) and 0 <= o < W
        # multiply-shift is monotone in the high word
        for hi in range(0, 1 << 32, 1 << 26):
            o = R.hook_fp_owner(hi << 32, W)
            assert o >= prev
            prev = o


def test_hooks_refuse_bad_arguments():
    L = R._lib()
    assert L.rmc_selftest_fp_slot(1, 6) == EMPTY            # mask + 1 not a power of two
    assert L.rmc_selftest_fp_owner(1, 0) < 0 and L.rmc_selftest_fp_owner(1, 65) < 0
    out = (ctypes.c_uint64 * 16)()
    u32 = ctypes.cast(out, ctypes.POINTER(ctypes.c_uint32))
    for slots in (0, 4, 7, 100, 1 << 25):
        assert not L.rmc_selftest_fpset_new(64, slots)      # refused before any device call
        assert b"slots" in L.rmc_last_error()
    assert not L.rmc_selftest_fpset_new(96, 64)
    # a null handle is refused by every hook that takes one
    assert L.rmc_selftest_fpset_insert(None, 0, out, out, 1, 0, out, u32, None) < 0
    assert L.rmc_selftest_fpset_lookup(None, out, 1, out) < 0
    assert L.rmc_selftest_fpset_grow(None, 16, u32) < 0
    assert L.rmc_selftest_fpset_reset_ranks(None, 0, 1) < 0
    assert L.rmc_selftest_fpset_dump(None, out, 16) < 0
    assert L.rmc_selftest_fpset_slots(None) < 0
    assert b"rmc_selftest_fpset" in L.rmc_last_error()
    assert L.rmc_selftest_owner_partition(out, out, u32, 1, 65, out, u32, u32) < 0
    assert L.rmc_selftest_owner_partition(out, out, u32, 0, 2, out, u32, u32) < 0
    off, cnt = (ctypes.c_uint32 * 2)(0, 5), (ctypes.c_uint32 * 2)(4, 4)   # a gap between the parents' ranges
    assert L.rmc_selftest_tile_dedup(off, cnt, 2, out, out, u32, 8) < 0


# ------------------------------------------------------------- the reference
def test_reference_rule():
    r = RefSet()
    assert r.apply([1, 2, 1], [30, 20, 10], 0) == {1, 2}
    assert r.d == {1: 10, 2: 20}
    assert r.apply([1, 3, 3], [100, 120, 110], 100) == {3}   # 1 is an earlier level's: unchanged
    assert r.d == {1: 10, 2: 20, 3: 110}


def test_reference_preconditions():
    r = RefSet()
    with pytest.raises(AssertionError):
        r.apply([1, 2], [5, 5], 0)            # equal values in a batch
    with pytest.raises(AssertionError):
        r.apply([1], [5], 6)                  # a value below the floor
    r.apply([1], [50], 0)
    with pytest.raises(AssertionError):
        r.apply([2], [60], 40)                # an earlier value not below the floor


def test_scenarios_meet_the_preconditions():
    """Every scenario the builders emit passes RefSet.apply's assertions."""
    for batches in (R.scn_home_run(256, 253, 200), R.scn_interleaved(256, 254), R.scn_heavy_dup(256, "adjacent"),
                    R.scn_heavy_dup(256, 64), R.scn_heavy_dup(256, 256 * R.RECV_U), R.scn_three_levels(256),
                    R.scn_full(64)[0], [R.scn_overflow(64, 100)], R.scn_two_chunks(256)[:2]):
        r = RefSet()
        for keys, vals, floor in batches:
            r.apply(keys, vals, floor)
            assert len(set(v >> 16 for v in vals)) == len(vals)  # distinct ranks
    keys, vals, _ = R.scn_heavy_dup(256, 64)[0]
    assert len(keys) == 4096 and len(set(keys)) == 37
    assert all(keys[j] == keys[j + 64] for j in range(4096 - 64))
    keys, _, _ = R.scn_heavy_dup(256, 1024)[0]
    assert all(keys[j] == keys[j + 1024] for j in range(4096 - 1024))
