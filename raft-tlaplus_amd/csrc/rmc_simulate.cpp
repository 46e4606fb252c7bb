// rmc_simulate.cpp — TLC's random simulation mode (`-simulate`) on the GPU:
// SURVEY.md §8f rank 2, "the author's recommended mode for the specs too big
// to exhaust" (flexible-raft/FlexibleRaft.cfg:5, pull-raft/KRaftWithReconfig.cfg:5).
//
// Rounds of `walkers` random behaviours run in parallel (k_simulate, one lane
// per behaviour), each from Init for at most `depth` steps, choosing every
// step uniformly among the enabled successors; invariants are checked on every
// state.  The run stops at the first violation / evaluation error (its
// behaviour is replayed on the host into a TLC-format trace), when `behaviors`
// behaviours have been generated, or after `seconds`.
#include <chrono>
#include <cstring>
#include <string>
#include <vector>
#include "rmc_internal.h"

using namespace rmc;

namespace rmcx {

// The message slots a simulation packs rows to, and the seed of round `round`
// (shared with the test hook rmc_selftest_simulate_round, which must make the
// launch simulate_impl makes).
static uint32_t sim_kmax(const rmc_model* m, const rmc_options* opt) {
  const uint32_t kmax = opt->msg_cap_K ? opt->msg_cap_K : (m->kmax_user ? m->kmax_user : default_kmax(m->M));
  return kmax > 120 ? 120 : kmax;
}
static unsigned long long sim_round_seed(unsigned long long seed, unsigned long long round) {
  return seed + 0x9E3779B97F4A7C15ULL * (round + 1);
}

static int simulate_impl(rmc_model* m, const rmc_options* opt, unsigned long long walkers, unsigned depth,
                         unsigned long long seed, unsigned long long behaviors, double seconds, rmc_result* res) {
  auto t0 = std::chrono::steady_clock::now();
  Model& M = m->M;
  finalize_model(m, sim_kmax(m, opt));
  HIPCHK(upload_model(M));
  const size_t W = (size_t)M.words;
  res->state_bytes = (uint32_t)(W * 4);
  m->levels.clear();
  m->trace_states.clear();
  m->trace_actions.clear();
  std::vector<uint32_t> init = init_state(M);
  std::string message;
  {
    int err = 0;
    int bad = host_check_invariants(M, init.data(), &err);
    if (err || bad >= 0) {
      res->status = err ? 2 : 1;
      if (!err) snprintf(res->violated, sizeof res->violated, "%s", m->inv_names[bad].c_str());
      replay_trace(m, {}, -1, res->status, message, res);
      res->generated = 1;
      res->distinct = 1;
      res->depth = 1;
      return 0;
    }
  }
  hipStream_t stream;
  HIPCHK(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
  DevBuf dinit, binds, counters, ssb, stb;
  dinit.ensure(W * 4);
  binds.ensure(walkers * depth * 2);
  counters.ensure(16);
  ssb.ensure(sizeof(SimStatus));
  stb.ensure(sizeof(DevStatus));
  HIPCHK(hipMemcpyAsync(dinit.p, init.data(), W * 4, hipMemcpyHostToDevice, stream));
  HIPCHK(hipMemsetAsync(counters.p, 0, 16, stream));
  {
    SimStatus s0;
    memset(&s0, 0, sizeof s0);
    s0.key = ~0ULL;
    HIPCHK(hipMemcpyAsync(ssb.p, &s0, sizeof s0, hipMemcpyHostToDevice, stream));
  }
  DevStatus hst;
  memset(&hst, 0, sizeof hst);
  hst.err_key = hst.inv_err_key = hst.viol_key = ~0ULL;
  hst.cap_flags = 0;
  hst.max_msgs = 0;
  HIPCHK(hipMemcpyAsync(stb.p, &hst, sizeof hst, hipMemcpyHostToDevice, stream));
  unsigned long long done = 0, generated = 0;
  unsigned long long round = 0;
  SimStatus ss;
  memset(&ss, 0, sizeof ss);
  ss.key = ~0ULL;
  int status = 0;
  unsigned long long cnt[2] = {0, 0};
  while (done < behaviors) {
    unsigned long long n = std::min(walkers, behaviors - done);
    unsigned long long rseed = sim_round_seed(seed, round);
    launch_simulate(M.spec, M.N, dinit.as<uint32_t>(), n, depth, rseed, binds.as<uint16_t>(),
                    counters.as<unsigned long long>(), ssb.as<SimStatus>(), stb.as<DevStatus>(), (int)W, stream);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(&ss, ssb.p, sizeof ss, hipMemcpyDeviceToHost, stream));
    HIPCHK(hipMemcpyAsync(&hst, stb.p, sizeof hst, hipMemcpyDeviceToHost, stream));
    HIPCHK(hipMemcpyAsync(cnt, counters.p, 16, hipMemcpyDeviceToHost, stream));
    HIPCHK(hipStreamSynchronize(stream));
    if (ss.key != ~0ULL) {
      ss.stop = (unsigned)(ss.key & 3u);
      ss.steps = (unsigned)((ss.key >> 2) & 0x3FFFFu);
      ss.walker = ss.key >> 20;
    }
    done += n;
    round++;
    if (hst.cap_flags) {
      int e = 0;
      while (!((hst.cap_flags >> e) & 1)) e++;
      if (e == E_CAP_MSG && !opt->msg_cap_K && M.kmax < 120) {
        m->kmax_user = std::min(120u, (uint32_t)M.kmax * 2);
        HIPCHK(hipStreamDestroy(stream));
        return 1;
      }
      status = 3;
      message = "capacity overflow in simulation (code " + std::to_string(e) + ")";
      break;
    }
    if (ss.stop) break;
    if (seconds > 0 && std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() >= seconds) break;
  }
  generated = done + cnt[0];  // initial states + steps
  if (ss.stop) {
    std::vector<uint16_t> b(ss.steps);
    HIPCHK(hipMemcpy(b.data(), binds.as<uint16_t>() + ss.walker * depth, ss.steps * 2, hipMemcpyDeviceToHost));
    std::vector<int> chain(b.begin(), b.end());
    int last_b = -1;
    if (ss.stop == 1) {
      status = 1;
    } else if (ss.stop == 2) {
      status = 2;
      last_b = chain.back();
      chain.pop_back();
      message = "evaluation error in the next-state relation (a sequence applied outside its domain)";
    } else {
      status = 2;
      message = "evaluation error while checking an invariant";
    }
    replay_trace(m, chain, last_b, status, message, res);
  }
  HIPCHK(hipStreamDestroy(stream));
  res->generated = generated;
  res->distinct = done;  // simulation: behaviours generated (TLC reports states generated and traces)
  res->depth = (uint32_t)(cnt[1] + 1);
  res->left_on_queue = 0;
  res->status = status;
  snprintf(res->message, sizeof res->message, "%s", message.c_str());
  res->seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  return 0;
}

}  // namespace rmcx

using namespace rmcx;

extern "C" int rmc_simulate(rmc_model* m, const rmc_options* o, uint64_t walkers, uint32_t depth, uint64_t seed,
                            uint64_t behaviors, double seconds, rmc_result* out) {
  if (!m || !out || !walkers || !depth || depth > 65535 || !behaviors) {
    set_last_error("bad argument");
    return -1;
  }
  rmc_options def;
  rmc_options_default(&def);
  if (!o) o = &def;
  memset(out, 0, sizeof *out);
  try {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) {
      set_last_error("no HIP device available: the raftmc GPU path requires an MI355X (gfx950)");
      return -4;
    }
    m->kmax_user = 0;
    int rc;
    while ((rc = simulate_impl(m, o, walkers, depth, seed, behaviors, seconds, out)) == 1) memset(out, 0, sizeof *out);
    return rc;
  } catch (std::exception& e) {
    set_last_error(e.what());
    return -5;
  }
}

// ---------------------------------------------------------------------------
// Test hooks (never reached from rmc_simulate / raftmc's product calls).
namespace rmcx {

// b is one of the bindings a state with nm DOMAIN elements has (binding_at)
static bool binding_in_range(const Model& M, int b, int nm) {
  if (b < 0) return false;
  if (b < M.nfixed + nm) return true;
  for (int j = 0; j < M.nmsgc; j++) {
    const int base = M.nfixed + MSGC_STRIDE * (1 + M.msgc_q[j]);
    if (b >= base && b < base + nm) return true;
  }
  return false;
}

// Does state S have an enabled binding (an evaluation error counts: TLC would stop on it)?
static bool host_has_successor(const Model& M, const uint32_t* S, uint32_t* tmp) {
  const int nm = h_nmsg(S[0]), B = nbindings(M, nm);
  for (int x = 0; x < B; x++) {
    int err = 0;
    if (host_eval_apply(M, S, binding_at(M, x, nm), tmp, nullptr, nullptr, &err) == 1) return true;
  }
  return false;
}

}  // namespace rmcx

// Test hook only: the words of this model's packed rows in a simulation with these options.
extern "C" int rmc_selftest_simulate_words(rmc_model* m, const rmc_options* o) {
  if (!m) return -1;
  rmc_options def;
  rmc_options_default(&def);
  if (!o) o = &def;
  try {
    m->kmax_user = 0;
    finalize_model(m, sim_kmax(m, o));
    return m->M.words;
  } catch (std::exception& e) {
    set_last_error(e.what());
    return -1;
  }
}

// Test hook only: round `round` of rmc_simulate(m, o, walkers, depth, seed, ..)
// as one launch (the same row packing, model upload and round seed), returning
// what every walker did: its recorded bindings (binds_out[w * depth ..], the
// first steps_out[w] of them are its behaviour), its step count and, if
// rows_out is not null, its final packed row (rows_out[w * words ..], words =
// rmc_selftest_simulate_words).  If host_mismatch_out (8 values) is not null
// every walker is then replayed on the host from init_state through
// host_eval_apply, as replay_trace does, and the hook reports (count, first
// walker) of:
//   [0,1] a recorded binding the host does not find enabled,
//   [2,3] a host final row that differs from the device's (the words up to the last message),
//   [4,5] a walker that stopped before `depth` with no stop kind whose host final state has a successor,
//   [6,7] a host invariant failure (or evaluation error) the device did not report as this
//         walker's stop, or one it reported that the host does not find.
// Returns the round's status as rmc_simulate would report it (0 ok, 1
// invariant violated, 2 evaluation error, 3 capacity overflow; no retry with
// more message slots here), negative on an API error.
extern "C" int rmc_selftest_simulate_round(rmc_model* m, const rmc_options* o, uint64_t walkers, uint32_t depth,
                                           uint64_t seed, uint64_t round, uint16_t* binds_out, uint32_t* steps_out,
                                           uint32_t* rows_out, uint64_t* host_mismatch_out) {
  if (!m || !walkers || !depth || depth > 65535 || !binds_out || !steps_out) {
    set_last_error("bad argument");
    return -1;
  }
  rmc_options def;
  rmc_options_default(&def);
  if (!o) o = &def;
  hipStream_t stream = nullptr;
  try {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) {
      set_last_error("no HIP device available: the raftmc GPU path requires an MI355X (gfx950)");
      return -4;
    }
    m->kmax_user = 0;
    Model& M = m->M;
    finalize_model(m, sim_kmax(m, o));
    HIPCHK(upload_model(M));
    const size_t W = (size_t)M.words;
    const std::vector<uint32_t> init = init_state(M);
    DevBuf dinit, binds, counters, ssb, stb, dsteps, drows;
    dinit.ensure(W * 4);
    binds.ensure(walkers * depth * 2);
    counters.ensure(16);
    ssb.ensure(sizeof(SimStatus));
    stb.ensure(sizeof(DevStatus));
    dsteps.ensure(walkers * 4);
    const bool want_rows = rows_out || host_mismatch_out;
    if (want_rows) drows.ensure(walkers * W * 4);
    HIPCHK(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
    HIPCHK(hipMemcpyAsync(dinit.p, init.data(), W * 4, hipMemcpyHostToDevice, stream));
    HIPCHK(hipMemsetAsync(counters.p, 0, 16, stream));
    // unwritten binding slots read as 0xFFFF, never as a binding of an earlier call
    HIPCHK(hipMemsetAsync(binds.p, 0xFF, walkers * depth * 2, stream));
    SimStatus ss;
    memset(&ss, 0, sizeof ss);
    ss.key = ~0ULL;
    HIPCHK(hipMemcpyAsync(ssb.p, &ss, sizeof ss, hipMemcpyHostToDevice, stream));
    DevStatus hst;
    memset(&hst, 0, sizeof hst);
    hst.err_key = hst.inv_err_key = hst.viol_key = ~0ULL;
    HIPCHK(hipMemcpyAsync(stb.p, &hst, sizeof hst, hipMemcpyHostToDevice, stream));
    launch_simulate(M.spec, M.N, dinit.as<uint32_t>(), walkers, depth, sim_round_seed(seed, round),
                    binds.as<uint16_t>(), counters.as<unsigned long long>(), ssb.as<SimStatus>(),
                    stb.as<DevStatus>(), (int)W, stream, dsteps.as<uint32_t>(),
                    want_rows ? drows.as<uint32_t>() : nullptr);
    HIPCHK(hipGetLastError());
    std::vector<uint32_t> rows_host;
    uint32_t* rows = rows_out;
    if (want_rows && !rows) {
      rows_host.resize(walkers * W);
      rows = rows_host.data();
    }
    HIPCHK(hipMemcpyAsync(&ss, ssb.p, sizeof ss, hipMemcpyDeviceToHost, stream));
    HIPCHK(hipMemcpyAsync(&hst, stb.p, sizeof hst, hipMemcpyDeviceToHost, stream));
    HIPCHK(hipMemcpyAsync(binds_out, binds.p, walkers * depth * 2, hipMemcpyDeviceToHost, stream));
    HIPCHK(hipMemcpyAsync(steps_out, dsteps.p, walkers * 4, hipMemcpyDeviceToHost, stream));
    if (want_rows) HIPCHK(hipMemcpyAsync(rows, drows.p, walkers * W * 4, hipMemcpyDeviceToHost, stream));
    HIPCHK(hipStreamSynchronize(stream));
    HIPCHK(hipStreamDestroy(stream));
    stream = nullptr;
    unsigned long long stop_walker = ~0ULL;
    unsigned stop_kind = 0, stop_steps = 0;
    if (ss.key != ~0ULL) {
      stop_kind = (unsigned)(ss.key & 3u);
      stop_steps = (unsigned)((ss.key >> 2) & 0x3FFFFu);
      stop_walker = ss.key >> 20;
    }
    const int status = hst.cap_flags ? 3 : stop_kind == 1 ? 1 : stop_kind ? 2 : 0;
    if (!host_mismatch_out) return status;
    uint64_t* mm = host_mismatch_out;
    for (int k = 0; k < 8; k++) mm[k] = 0;
    auto note = [&](int kind, uint64_t w) {
      if (!mm[2 * kind]++) mm[2 * kind + 1] = w;
    };
    std::vector<uint32_t> s(W), t(W);
    for (uint64_t w = 0; w < walkers; w++) {
      const unsigned n = steps_out[w];
      const uint16_t* b = binds_out + w * depth;
      s = init;
      // the host's own stop of this walker: kind (as SimStatus::key) after `hsteps` steps
      unsigned hkind = 0, hsteps = 0;
      bool bad_binding = n > depth;
      for (unsigned k = 0; k < n && !bad_binding && !hkind; k++) {
        int err = 0;
        if (!binding_in_range(M, b[k], h_nmsg(s[0])) ||
            host_eval_apply(M, s.data(), b[k], t.data(), nullptr, nullptr, &err) != 1) {
          bad_binding = true;
          break;
        }
        if (err) {  // an evaluation error in Next (or a row out of message slots): no successor state
          hkind = 2;
          hsteps = k + 1;
          break;
        }
        s = t;
        int ierr = 0;
        const int viol = host_check_invariants(M, s.data(), &ierr);
        if (ierr || viol >= 0) {
          hkind = ierr ? 3 : 1;
          hsteps = k + 1;
        }
      }
      if (bad_binding) {
        note(0, w);
        continue;
      }
      // the device reports the failing behaviour with the lowest walker index
      const bool dev_stop_here = w == stop_walker;
      if (hkind) {
        if (hsteps != n || stop_walker > w || (dev_stop_here && (stop_kind != hkind || stop_steps != hsteps))) note(3, w);
      } else if (dev_stop_here) {
        note(3, w);
      }
      const size_t live = 1 + 4 * (size_t)M.N + (size_t)h_nmsg(s[0]);
      if (memcmp(s.data(), rows + w * W, std::min(live, W) * 4) != 0) note(1, w);
      if (!hkind && n < depth && !hst.cap_flags && host_has_successor(M, s.data(), t.data())) note(2, w);
    }
    return status;
  } catch (std::exception& e) {
    if (stream) (void)hipStreamDestroy(stream);
    set_last_error(e.what());
    return -5;
  }
}

// Test hook only (never called by rmc_check / rmc_simulate): load the binding
// chain binds[0..n) into the model's trace through replay_trace, as after a
// violation, so rmc_trace_module / rmc_trace_state give the behaviour's states.
// Returns the number of states (n + 1); -1 with rmc_last_error set if a
// binding of the chain is not enabled in its state.
extern "C" int rmc_selftest_replay_binds(rmc_model* m, const uint16_t* binds, int n) {
  if (!m || n < 0 || (n && !binds)) {
    set_last_error("bad argument");
    return -1;
  }
  try {
    finalize_model(m, m->kmax_user ? m->kmax_user : default_kmax(m->M));
    const Model& M = m->M;
    std::vector<uint32_t> s = init_state(M), t(M.words, 0u);
    std::vector<int> chain(binds, binds + n);
    for (int k = 0; k < n; k++) {
      int err = 0;
      if (!binding_in_range(M, chain[k], h_nmsg(s[0])) ||
          host_eval_apply(M, s.data(), chain[k], t.data(), nullptr, nullptr, &err) != 1 || err) {
        set_last_error("trace replay: binding " + std::to_string(chain[k]) + " at step " + std::to_string(k + 1) +
                       " is not enabled");
        return -1;
      }
      s = t;
    }
    m->trace_states.clear();
    m->trace_actions.clear();
    rmc_result res;
    memset(&res, 0, sizeof res);
    std::string msg;
    replay_trace(m, chain, -1, 0, msg, &res);
    return (int)m->trace_states.size();
  } catch (std::exception& e) {
    set_last_error(e.what());
    return -1;
  }
}
