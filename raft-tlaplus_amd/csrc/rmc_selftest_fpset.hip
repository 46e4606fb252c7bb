// rmc_selftest_fpset.hip — test hooks into the fingerprint set (rmc_fpset.h)
// and its companion kernels (rmc_kernels.hip), for tests/test_gpu_fpset.py.
//
// The hooks run the production code, not copies: thin kernels whose threads
// call fpset_insert / fpset_insert128 / fpset_value as k_expand does, and the
// host launchers of rmc_engine.h (launch_insert_recv, launch_mark_recv,
// launch_rehash, launch_reset_ranks, launch_owner_count + launch_scan +
// launch_bucket, launch_tile_dedup) exactly as the drivers call them.  A test
// builds keys for chosen home slots, inserts them on a small table, copies the
// table back and compares it with a dictionary.
//
// Built into librmc_selftest.so, a library of its own that links against
// librmc.so for the launchers (Makefile): librmc.so is the same with or
// without these hooks.  Not part of include/rmc.h.  Every hook
// checks its arguments before anything is launched: a bad argument returns a
// negative value with rmc_last_error set.
#include <hip/hip_runtime.h>
#include <string>
#include <vector>
#include "rmc_internal.h"
#include "rmc_fpset.h"

using namespace rmc;
using rmcx::set_last_error;

namespace {

constexpr uint64_t ST_MAGIC = 0x7365746670735446ULL;
constexpr uint64_t ST_MAX_SLOTS = 1ULL << 24, ST_MAX_N = 1ULL << 22;
// The table is allocated with ST_GUARD more entries behind its last slot.  They
// are no part of the set (mask = slots - 1) and must stay EMPTY: a probe that
// steps past the last slot without wrapping shows in the dump instead of
// writing to foreign memory.
constexpr uint64_t ST_GUARD = 16;

__global__ __launch_bounds__(256) void k_st_insert(unsigned long long* T, unsigned long long mask,
                                                   const unsigned long long* __restrict__ fps,
                                                   const unsigned long long* __restrict__ vals, unsigned long long n,
                                                   unsigned long long floor, unsigned long long* __restrict__ out,
                                                   DevStatus* st) {
  const unsigned long long stride = (unsigned long long)gridDim.x * blockDim.x;
  for (unsigned long long j = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; j < n; j += stride)
    out[j] = fpset_insert(T, mask, fps[j], vals[j], floor, st);
}
__global__ __launch_bounds__(256) void k_st_insert128(unsigned long long* T, unsigned long long mask,
                                                      const unsigned long long* __restrict__ fps,
                                                      const unsigned long long* __restrict__ vals,
                                                      unsigned long long n, unsigned long long floor,
                                                      unsigned long long* __restrict__ out, DevStatus* st) {
  const unsigned long long stride = (unsigned long long)gridDim.x * blockDim.x;
  for (unsigned long long j = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; j < n; j += stride)
    out[j] = fpset_insert128(T, mask, Fp128{fps[2 * j], fps[2 * j + 1]}, vals[j], floor, st);
}
__global__ __launch_bounds__(256) void k_st_lookup(const unsigned long long* T, unsigned long long mask,
                                                   const unsigned long long* __restrict__ fps, unsigned long long n,
                                                   unsigned long long* __restrict__ out) {
  const unsigned long long stride = (unsigned long long)gridDim.x * blockDim.x;
  for (unsigned long long j = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; j < n; j += stride)
    out[j] = fpset_value(T, mask, fps[j]);
}

// a device buffer freed at scope exit
struct Dev {
  void* p = nullptr;
  explicit Dev(size_t bytes) { HIPCHK(hipMalloc(&p, bytes ? bytes : 16)); }
  ~Dev() { if (p) (void)hipFree(p); }
  Dev(const Dev&) = delete;
  Dev& operator=(const Dev&) = delete;
  template <class T>
  T* as() const { return (T*)p; }
};

struct FpSetTest {
  uint64_t magic = ST_MAGIC;
  int ew = 2;  // entry width in words: 2 (fp_bits 64), 4 (fp_bits 128)
  uint64_t slots = 0;
  unsigned long long* T = nullptr;
  DevStatus* st = nullptr;
  // the last recv-path batch, kept on the device for mark_recv
  unsigned long long *recv = nullptr, *recv_slot = nullptr;
  uint64_t recv_n = 0;
  bool have_recv = false;
  ~FpSetTest() {
    magic = 0;
    if (T) (void)hipFree(T);
    if (st) (void)hipFree(st);
    if (recv) (void)hipFree(recv);
    if (recv_slot) (void)hipFree(recv_slot);
  }
};

bool pow2(uint64_t x) { return x && !(x & (x - 1)); }
FpSetTest* handle(void* h) {
  FpSetTest* t = (FpSetTest*)h;
  return t && t->magic == ST_MAGIC ? t : nullptr;
}
int bad(const char* what) {
  set_last_error(std::string("rmc_selftest_fpset: ") + what);
  return -1;
}
bool have_device() {
  int ndev = 0;
  return hipGetDeviceCount(&ndev) == hipSuccess && ndev >= 1;
}
void reset_status(DevStatus* st) { HIPCHK(hipMemset(st, 0, sizeof(DevStatus))); }
unsigned read_flags(const DevStatus* st, unsigned long long* hidden = nullptr) {
  DevStatus h;
  HIPCHK(hipMemcpy(&h, st, sizeof h, hipMemcpyDeviceToHost));
  if (hidden) *hidden = h.hidden_coll;
  return h.cap_flags;
}
unsigned grid_for_n(uint64_t n) { return (unsigned)((n + 255) / 256); }

template <class F>
int guarded(F f) {
  try {
    return f();
  } catch (std::exception& e) {
    set_last_error(e.what());
    return -5;
  }
}

}  // namespace

// ---- host-only helpers: the slot and owner functions the kernels use
extern "C" uint64_t rmc_selftest_fp_slot(uint64_t fp, uint64_t mask) {
  if (!pow2(mask + 1) || mask == 0) return ~0ULL;
  return fp_slot(fp, mask);
}
extern "C" int rmc_selftest_fp_owner(uint64_t fp, int W) {
  if (W < 1 || W > 64) return -1;
  return fp_owner(fp, W);
}

// ---- the table
extern "C" void* rmc_selftest_fpset_new(int fp_bits, uint64_t slots) {
  if ((fp_bits != 64 && fp_bits != 128) || !pow2(slots) || slots < 8 || slots > ST_MAX_SLOTS) {
    bad("new: fp_bits is 64 or 128, slots a power of two in [8, 2^24]");
    return nullptr;
  }
  if (!have_device()) {
    bad("no HIP device available");
    return nullptr;
  }
  FpSetTest* t = nullptr;
  try {
    t = new FpSetTest;
    t->ew = fp_bits == 128 ? 4 : 2;
    t->slots = slots;
    HIPCHK(hipMalloc((void**)&t->T, (slots + ST_GUARD) * t->ew * 8));
    HIPCHK(hipMalloc((void**)&t->st, sizeof(DevStatus)));
    HIPCHK(hipMemset(t->T, 0xFF, (slots + ST_GUARD) * t->ew * 8));
    reset_status(t->st);
    HIPCHK(hipDeviceSynchronize());
    return t;
  } catch (std::exception& e) {
    delete t;
    set_last_error(e.what());
    return nullptr;
  }
}
extern "C" void rmc_selftest_fpset_free(void* h) {
  FpSetTest* t = handle(h);
  if (!t) return;
  (void)hipDeviceSynchronize();
  delete t;
}
extern "C" int64_t rmc_selftest_fpset_slots(void* h) {
  FpSetTest* t = handle(h);
  return t ? (int64_t)t->slots : (int64_t)bad("slots: bad handle");
}

// path 0: a thread per key calls fpset_insert (fp_bits 64: fps[n]) or
// fpset_insert128 (fp_bits 128: fps[2n], first word then second);
// path 1 (fp_bits 64 only): launch_insert_recv on (fp, val) records.
// out_slots[j] = the slot insert j returned (~0: none); out_raw (path 1, may be
// null) = k_insert_recv's slot words as written; *out_cap_flags = the status
// flags of this batch alone.
extern "C" int rmc_selftest_fpset_insert(void* h, int path, const uint64_t* fps, const uint64_t* vals, uint64_t n,
                                         uint64_t floor, uint64_t* out_slots, uint32_t* out_cap_flags,
                                         uint64_t* out_raw) {
  FpSetTest* t = handle(h);
  if (!t) return bad("insert: bad handle");
  if (path != 0 && path != 1) return bad("insert: path is 0 (device insert) or 1 (recv insert)");
  if (path == 1 && t->ew != 2) return bad("insert: the recv path stores 64-bit fingerprints");
  if (n > ST_MAX_N) return bad("insert: n too large");
  if (!out_cap_flags || (n && (!fps || !vals || !out_slots))) return bad("insert: null buffer");
  return guarded([&]() {
    const size_t kw = t->ew == 4 ? 2 : 1;
    reset_status(t->st);
    std::vector<unsigned long long> out(n);
    if (path == 0) {
      Dev dfp(n * kw * 8), dval(n * 8), dout(n * 8);
      if (n) {
        HIPCHK(hipMemcpy(dfp.p, fps, n * kw * 8, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(dval.p, vals, n * 8, hipMemcpyHostToDevice));
        if (t->ew == 2)
          hipLaunchKernelGGL(k_st_insert, dim3(grid_for_n(n)), dim3(256), 0, 0, t->T, t->slots - 1,
                             dfp.as<unsigned long long>(), dval.as<unsigned long long>(), n, floor,
                             dout.as<unsigned long long>(), t->st);
        else
          hipLaunchKernelGGL(k_st_insert128, dim3(grid_for_n(n)), dim3(256), 0, 0, t->T, t->slots - 1,
                             dfp.as<unsigned long long>(), dval.as<unsigned long long>(), n, floor,
                             dout.as<unsigned long long>(), t->st);
        HIPCHK(hipGetLastError());
        HIPCHK(hipDeviceSynchronize());
        HIPCHK(hipMemcpy(out.data(), dout.p, n * 8, hipMemcpyDeviceToHost));
      }
      for (uint64_t j = 0; j < n; j++) out_slots[j] = out[j];
    } else {
      std::vector<unsigned long long> rec(2 * n);
      for (uint64_t j = 0; j < n; j++) {
        rec[2 * j] = fps[j];
        rec[2 * j + 1] = vals[j];
      }
      if (t->recv) HIPCHK(hipFree(t->recv));
      if (t->recv_slot) HIPCHK(hipFree(t->recv_slot));
      t->recv = t->recv_slot = nullptr;
      t->have_recv = false;
      HIPCHK(hipMalloc((void**)&t->recv, n ? 2 * n * 8 : 16));
      HIPCHK(hipMalloc((void**)&t->recv_slot, n ? n * 8 : 16));
      if (n) {
        HIPCHK(hipMemcpy(t->recv, rec.data(), 2 * n * 8, hipMemcpyHostToDevice));
        HIPCHK(hipMemset(t->recv_slot, 0xEE, n * 8));  // a record the kernel skipped shows
      }
      launch_insert_recv(t->recv, n, t->T, t->slots - 1, floor, t->recv_slot, t->st, 0);
      HIPCHK(hipGetLastError());
      HIPCHK(hipDeviceSynchronize());
      if (n) HIPCHK(hipMemcpy(out.data(), t->recv_slot, n * 8, hipMemcpyDeviceToHost));
      for (uint64_t j = 0; j < n; j++) {
        if (out_raw) out_raw[j] = out[j];
        out_slots[j] = (out[j] & CAND_DUP) ? ~0ULL : (out[j] & CAND_SLOT_MASK);
      }
      t->recv_n = n;
      t->have_recv = true;
    }
    *out_cap_flags = read_flags(t->st);
    return 0;
  });
}

// fpset_value of every key (fp_bits 64)
extern "C" int rmc_selftest_fpset_lookup(void* h, const uint64_t* fps, uint64_t n, uint64_t* out_vals) {
  FpSetTest* t = handle(h);
  if (!t) return bad("lookup: bad handle");
  if (t->ew != 2) return bad("lookup: fpset_value reads 64-bit fingerprints");
  if (n > ST_MAX_N) return bad("lookup: n too large");
  if (n && (!fps || !out_vals)) return bad("lookup: null buffer");
  if (!n) return 0;
  return guarded([&]() {
    Dev dfp(n * 8), dout(n * 8);
    HIPCHK(hipMemcpy(dfp.p, fps, n * 8, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_st_lookup, dim3(grid_for_n(n)), dim3(256), 0, 0, t->T, t->slots - 1,
                       dfp.as<unsigned long long>(), n, dout.as<unsigned long long>());
    HIPCHK(hipGetLastError());
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(out_vals, dout.p, n * 8, hipMemcpyDeviceToHost));
    return 0;
  });
}

// launch_rehash into a fresh table of new_slots, as the drivers grow the set;
// *out_cap_flags = the rehash's status flags
extern "C" int rmc_selftest_fpset_grow(void* h, uint64_t new_slots, uint32_t* out_cap_flags) {
  FpSetTest* t = handle(h);
  if (!t) return bad("grow: bad handle");
  if (!pow2(new_slots) || new_slots <= t->slots || new_slots > ST_MAX_SLOTS)
    return bad("grow: new_slots is a power of two above the current size, at most 2^24");
  if (!out_cap_flags) return bad("grow: null buffer");
  return guarded([&]() {
    unsigned long long* nt = nullptr;
    HIPCHK(hipMalloc((void**)&nt, (new_slots + ST_GUARD) * t->ew * 8));
    try {
      HIPCHK(hipMemset(nt, 0xFF, (new_slots + ST_GUARD) * t->ew * 8));
      reset_status(t->st);
      launch_rehash(t->T, t->slots, nt, new_slots - 1, t->st, 0, t->ew);
      HIPCHK(hipGetLastError());
      HIPCHK(hipDeviceSynchronize());
    } catch (...) {
      (void)hipFree(nt);
      throw;
    }
    (void)hipFree(t->T);
    t->T = nt;
    t->slots = new_slots;
    t->have_recv = false;  // the recorded slots are the old table's
    *out_cap_flags = read_flags(t->st);
    return 0;
  });
}

// launch_reset_ranks over the whole table: ranks in [lo, hi)
extern "C" int rmc_selftest_fpset_reset_ranks(void* h, uint64_t lo, uint64_t hi) {
  FpSetTest* t = handle(h);
  if (!t) return bad("reset_ranks: bad handle");
  if (lo > hi) return bad("reset_ranks: lo > hi");
  return guarded([&]() {
    launch_reset_ranks(t->T, t->slots, t->ew, lo, hi, 0);
    HIPCHK(hipGetLastError());
    HIPCHK(hipDeviceSynchronize());
    return 0;
  });
}

// launch_mark_recv over the last recv-path batch (n = its size)
extern "C" int rmc_selftest_fpset_mark_recv(void* h, uint64_t n, uint64_t floor, uint8_t* out_flags,
                                            uint64_t* out_newcount, uint64_t* out_hidden_coll) {
  FpSetTest* t = handle(h);
  if (!t) return bad("mark_recv: bad handle");
  if (!t->have_recv || n != t->recv_n) return bad("mark_recv: n is not the size of the last recv-path batch");
  if (!out_newcount || !out_hidden_coll || (n && !out_flags)) return bad("mark_recv: null buffer");
  return guarded([&]() {
    Dev dflag(n), dnew(8);
    if (n) HIPCHK(hipMemset(dflag.p, 0xEE, n));
    HIPCHK(hipMemset(dnew.p, 0, 8));
    reset_status(t->st);
    launch_mark_recv(t->recv, t->recv_slot, n, t->T, floor, dflag.as<uint8_t>(), dnew.as<unsigned long long>(),
                     t->st, 0);
    HIPCHK(hipGetLastError());
    HIPCHK(hipDeviceSynchronize());
    if (n) HIPCHK(hipMemcpy(out_flags, dflag.p, n, hipMemcpyDeviceToHost));
    unsigned long long nc = 0, hc = 0;
    HIPCHK(hipMemcpy(&nc, dnew.p, 8, hipMemcpyDeviceToHost));
    (void)read_flags(t->st, &hc);
    *out_newcount = nc;
    *out_hidden_coll = hc;
    return 0;
  });
}

// the whole table and the guard entries behind it, (slots + 16) * (2 or 4)
// words; returns the number of words
extern "C" int64_t rmc_selftest_fpset_dump(void* h, uint64_t* out_words, uint64_t cap_words) {
  FpSetTest* t = handle(h);
  if (!t) return bad("dump: bad handle");
  const uint64_t words = (t->slots + ST_GUARD) * t->ew;
  if (!out_words || cap_words < words) return bad("dump: buffer too small");
  return guarded([&]() {
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(out_words, t->T, words * 8, hipMemcpyDeviceToHost));
    return (int)words;
  });
}

// ---- sharded search: bucketing by owner, as rmc_sharded.cpp runs it
// (launch_owner_count, launch_scan over the owner-major block counts plus a
// closing zero, launch_bucket).  send_out[2n], perm_out[n], counts_out[W].
extern "C" int rmc_selftest_owner_partition(const uint64_t* cand_fp, const uint64_t* cand_val, const uint32_t* cand_ob,
                                            uint64_t n, int W, uint64_t* send_out, uint32_t* perm_out,
                                            uint32_t* counts_out) {
  if (W < 1 || W > 64) return bad("owner_partition: W is in [1, 64]");
  if (n < 1 || n > ST_MAX_N) return bad("owner_partition: n is in [1, 2^22]");
  if (!cand_fp || !cand_val || !cand_ob || !send_out || !perm_out || !counts_out)
    return bad("owner_partition: null buffer");
  if (!have_device()) return bad("no HIP device available");
  return guarded([&]() {
    const unsigned long long nb = bucket_blocks(n), nbw = nb * (unsigned long long)W;
    Dev dfp(n * 8), dval(n * 8), dob(n * 4), bcnt((nbw + 1) * 4), boff((nbw + 1) * 4), send(2 * n * 8), perm(n * 4);
    const size_t tb = scan_temp_bytes(nbw + 1);
    Dev tmp(tb);
    HIPCHK(hipMemcpy(dfp.p, cand_fp, n * 8, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(dval.p, cand_val, n * 8, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(dob.p, cand_ob, n * 4, hipMemcpyHostToDevice));
    HIPCHK(hipMemset(send.p, 0xFF, 2 * n * 8));
    HIPCHK(hipMemset(perm.p, 0xEE, n * 4));
    unsigned int* bc = bcnt.as<unsigned int>();
    HIPCHK(hipMemset(bc + nbw, 0, 4));
    launch_owner_count(dfp.as<unsigned long long>(), dob.as<uint32_t>(), n, W, bc, 0);
    HIPCHK(hipGetLastError());
    launch_scan(tmp.p, tb, bc, boff.as<uint32_t>(), nbw + 1, 0);
    HIPCHK(hipGetLastError());
    launch_bucket(dfp.as<unsigned long long>(), dval.as<unsigned long long>(), dob.as<uint32_t>(), n, W,
                  boff.as<unsigned int>(), send.as<unsigned long long>(), perm.as<uint32_t>(), 0);
    HIPCHK(hipGetLastError());
    HIPCHK(hipDeviceSynchronize());
    std::vector<unsigned int> off(nbw + 1);
    HIPCHK(hipMemcpy(off.data(), boff.p, (nbw + 1) * 4, hipMemcpyDeviceToHost));
    // owner o's segment starts at off[o * nb]; the total closes the last one
    for (int o = 0; o < W; o++) counts_out[o] = off[(size_t)(o + 1) * nb] - off[(size_t)o * nb];
    HIPCHK(hipMemcpy(send_out, send.p, 2 * n * 8, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(perm_out, perm.p, n * 4, hipMemcpyDeviceToHost));
    return 0;
  });
}

// ---- sharded search: launch_tile_dedup on one contiguous candidate range
// (parent p's candidates are [par_off[p], par_off[p] + par_n[p]), back to
// back, as k_expand lays them out); cand_val and cand_ob are changed in place.
extern "C" int rmc_selftest_tile_dedup(const uint32_t* par_off, const uint32_t* par_n, uint64_t nparents,
                                       const uint64_t* cand_fp, uint64_t* cand_val, uint32_t* cand_ob,
                                       uint64_t ncand) {
  if (nparents < 1 || nparents > (1ULL << 16)) return bad("tile_dedup: nparents is in [1, 65536]");
  if (ncand < 1 || ncand > ST_MAX_N) return bad("tile_dedup: ncand is in [1, 2^22]");
  if (!par_off || !par_n || !cand_fp || !cand_val || !cand_ob) return bad("tile_dedup: null buffer");
  uint64_t at = 0;
  for (uint64_t p = 0; p < nparents; p++) {
    if (par_off[p] != at) return bad("tile_dedup: the parents' candidate ranges are not back to back from 0");
    at += par_n[p];
    if (at > ncand) return bad("tile_dedup: a parent's candidates pass ncand");
  }
  if (!have_device()) return bad("no HIP device available");
  return guarded([&]() {
    Dev doff(nparents * 4), dn(nparents * 4), dfp(ncand * 8), dval(ncand * 8), dob(ncand * 4);
    HIPCHK(hipMemcpy(doff.p, par_off, nparents * 4, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(dn.p, par_n, nparents * 4, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(dfp.p, cand_fp, ncand * 8, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(dval.p, cand_val, ncand * 8, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(dob.p, cand_ob, ncand * 4, hipMemcpyHostToDevice));
    LevelArgs a{};
    a.nparents = nparents;
    a.par_off = doff.as<uint32_t>();
    a.par_n = dn.as<uint32_t>();
    launch_tile_dedup(a, dfp.as<unsigned long long>(), dval.as<unsigned long long>(), dob.as<uint32_t>(), 0);
    HIPCHK(hipGetLastError());
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(cand_val, dval.p, ncand * 8, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(cand_ob, dob.p, ncand * 4, hipMemcpyDeviceToHost));
    return 0;
  });
}
