// runlist.hip -- rd_run_list / rd_join_lanes (include/ramdsir.h): the step's launch list walked in C++, one call per segment,
// with the lane forks / joins as HIP events.  Host code only.
#include <hip/hip_runtime.h>
#include <string.h>
#include <stdlib.h>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <mutex>
#include <thread>
#include <vector>
#include <tuple>
#include <type_traits>
#include <utility>
#include "common.h"
#include "../../include/ramdsir.h"

thread_local hipEvent_t rd_tls_stop_event = nullptr;        // common.h rd_launch
thread_local int rd_tls_stop_used = 0;

namespace {

// Events for the cross-stream edges of the SINGLE-THREADED walk (record and wait are issued back to back by the caller).  An event can
// be recorded again as soon as the hipStreamWaitEvent that uses it has been enqueued (the wait captures the record it was called
// after), so a small ring per device is enough there.  Edges that pass through a lane worker thread use the worker's own pool
// (worker_event below), whose slots are reused only after the worker has executed the command that carries them.
constexpr int EV_RING = 64, EV_MAX_DEV = 16;
struct EvRing {
    hipEvent_t ev[EV_RING];
    int next = 0;
    bool ready = false;
};
EvRing g_rings[EV_MAX_DEV];

int next_event(hipEvent_t* out) {
    int dev = 0;
    RD_CHECK(hipGetDevice(&dev));
    if (dev < 0 || dev >= EV_MAX_DEV) return -1;
    EvRing& r = g_rings[dev];
    if (!r.ready) {
        for (int i = 0; i < EV_RING; ++i) RD_CHECK(hipEventCreateWithFlags(&r.ev[i], hipEventDisableTiming));
        r.ready = true;
    }
    *out = r.ev[r.next];
    r.next = (r.next + 1) % EV_RING;
    return 0;
}

// stream `to` waits for everything enqueued on `from` so far
int edge(hipStream_t from, hipStream_t to) {
    if (from == to) return 0;
    hipEvent_t e;
    const int err = next_event(&e);
    if (err) return err;
    RD_CHECK(hipEventRecord(e, from));
    RD_CHECK(hipStreamWaitEvent(to, e, 0));
    return 0;
}

#ifdef RD_DEBUG_SWITCHES
static int rd_switch_rl(const char* name) { const char* e = getenv(name); return e ? atoi(e) : 0; }
// Debug library, RD_POISON_LDS=1: in front of EVERY launch of a list a kernel fills the LDS of every CU (and the registers of the waves
// it runs) with a NaN pattern -- 0x7fc07fc0 is a NaN as fp32 and as two bf16, and 1e307-sized as half an fp64.  LDS and registers are
// not cleared between kernels: a launch that reads either before writing it normally sees what the previous kernel of the same process
// left there (repeatable when the process is alone on the GPU, arbitrary when it is not); with the poison it sees NaNs, and the losses show it.
__global__ __launch_bounds__(1024) void rd_poison_lds_kernel(int words) {
    extern __shared__ unsigned poison_smem[];
    for (int i = threadIdx.x; i < words; i += blockDim.x) poison_smem[i] = 0x7fc07fc0u;
    __syncthreads();
    if (poison_smem[(threadIdx.x * 7) % words] == 1u) poison_smem[0] = 2u;         // keep the stores alive
}
void poison_lds(void* st) {
    static int on = -1, cus = 0;
    if (on < 0) {
        on = rd_switch_rl("RD_POISON_LDS");
        hipDeviceProp_t pr;
        int dev = 0;
        (void)hipGetDevice(&dev);
        (void)hipGetDeviceProperties(&pr, dev);
        cus = pr.multiProcessorCount;
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&rd_poison_lds_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    }
    if (on != 1) return;
    // one 160 KB workgroup per CU (x2 so that every CU gets one even if some run two 80 KB... the second wave of workgroups overwrites again)
    rd_launch(rd_poison_lds_kernel, dim3(2 * cus), dim3(1024), 160 * 1024, (hipStream_t)st, 160 * 1024 / 4);
}
#endif

// One argument of an entry point from the 64-bit word rd_launch_t.a[] carries: pointers and integers as they are, a float from its bit
// pattern in the low 32 bits.
template <class T> T unpack(uint64_t v) {
    static_assert(std::is_pointer_v<T> || std::is_same_v<T, int> || std::is_same_v<T, int64_t> || std::is_same_v<T, float>);
    if constexpr (std::is_pointer_v<T>) return (T)(uintptr_t)v;
    else if constexpr (std::is_same_v<T, float>) return __builtin_bit_cast(float, (uint32_t)v);
    else return (T)(int64_t)v;
}
// One row per entry point of RD_LAUNCH_OPS (include/ramdsir.h): argument types and arity are the function's own signature minus the
// trailing stream.
struct OpRow {
    const char* name;
    int nargs;
    int (*call)(const uint64_t* a, void* st);
};
template <class... P, size_t... I> int unpack_and_call(int (*fn)(P...), const uint64_t* a, void* st, std::index_sequence<I...>) {
    static_assert(sizeof...(I) <= RD_LAUNCH_MAX_ARGS && std::is_same_v<std::tuple_element_t<sizeof...(I), std::tuple<P...>>, void*>);
    return fn(unpack<std::tuple_element_t<I, std::tuple<P...>>>(a[I])..., st);
}
template <class... P> constexpr int arity(int (*)(P...)) { return (int)sizeof...(P) - 1; }
template <auto Fn> int thunk(const uint64_t* a, void* st) { return unpack_and_call(Fn, a, st, std::make_index_sequence<arity(Fn)>{}); }
#define RD_OP_ROW(suffix, fn) {#fn, arity(&fn), thunk<&fn>},
constexpr OpRow OPS[] = {RD_LAUNCH_OPS(RD_OP_ROW)};
static_assert(RD_OP_CONV == 10 && RD_OP_RAM_MIX == 33 && RD_OP_END_ - RD_OP_CONV == sizeof(OPS) / sizeof(OPS[0]), "the op codes are ABI");

// the entry's row; null for an unknown op or a wrong argument count
const OpRow* row_of(const rd_launch_t& o) {
    const bool known = o.op >= RD_OP_CONV && o.op < RD_OP_END_ && o.nargs == OPS[o.op - RD_OP_CONV].nargs;
    return known ? &OPS[o.op - RD_OP_CONV] : nullptr;
}
int call(const rd_launch_t& o, void* st) {
#ifdef RD_DEBUG_SWITCHES
    poison_lds(st);
#endif
    const OpRow* r = row_of(o);
    return r ? r->call(o.a, st) : -1;
}

}  // namespace

namespace {

// ------------------------------------------------------------------------------------------------ lane worker threads
// A launch costs the host ~2.4 us inside the HIP runtime whoever calls it, so one thread cannot enqueue the step's ~305 kernels in less
// than ~0.85 ms.  With rd_run_list_threads(1) every lane k > 0 has a worker thread that enqueues that lane's entries while the calling
// thread enqueues lane 0's and records the events of the cross-lane edges:
//   fork / wait_main edge  the caller records an event at its position on the main stream, then hands the lane {wait for that event}:
//                          the event is recorded before the worker can see the command, so the worker never waits on the host side;
//   join                   the caller hands the lane {record an event}, waits (host side, bounded) until the worker has executed it and
//                          makes the main stream wait for the event.
// Stream order per lane is the list order, exactly as in the single-threaded walk: the GPU sees the same dependency graph.  Before
// rd_run_list returns every worker has drained its queue (everything is enqueued; descriptors may be changed by the caller afterwards).
struct Cmd {
    int kind;            // 0 launch ops[idx]; 1 stream waits for ev; 2 record ev on the stream; 3 new call: device / ops / stream
    int idx;
    hipEvent_t ev;
    const rd_launch_t* ops;
    hipStream_t stream;
};
constexpr unsigned RING = 4096;
// Events of the edges that go THROUGH a worker come from a pool of the worker's own (not from the per-device ring above): the caller
// records (or reserves) an event and the worker uses it later, asynchronously, so a slot may only be reused once the worker has
// executed the command that carries it.  ev_used counts those commands as the worker executes them; the caller hands out slot
// ev_issued % EV_POOL only while ev_issued - ev_used < EV_POOL (it waits otherwise: the worker is behind by a whole pool).
constexpr unsigned EV_POOL = 256;
struct Worker {
    Cmd ring[RING];
    std::atomic<unsigned> head{0}, tail{0};     // single producer (the caller), single consumer (the worker)
    std::atomic<int> err{0};
    std::atomic<int> asleep{0};
    std::atomic<int> poisoned{0};               // a push / drain timed out: the worker discards what it still holds and is never used again
    std::atomic<unsigned> ev_used{0};
    unsigned ev_issued = 0;                     // caller side only
    hipEvent_t evpool[EV_POOL];
    bool ev_ready = false;
    std::mutex m;
    std::condition_variable cv;
};
Worker* g_workers[EV_MAX_DEV][32] = {};          // keyed by (device, lane): two devices never share a single-producer ring
std::mutex g_workers_mutex;
std::atomic<int> g_threads_enabled{0};
std::atomic<int> g_bind_fork_events{1};                     // rd_run_list_bind_fork_events
std::atomic<long long> g_forks_bound{0}, g_forks_recorded{0};   // rd_run_list_fork_counts

void worker_main(Worker* w) {
    const rd_launch_t* ops = nullptr;
    hipStream_t stream = nullptr;
    for (;;) {
        unsigned h = w->head.load(std::memory_order_relaxed);
        int spins = 0;
        while (w->tail.load(std::memory_order_acquire) == h) {
            if (++spins < 20000) { __builtin_ia32_pause(); continue; }
            std::unique_lock<std::mutex> lk(w->m);                // nothing for ~100 us: sleep until the next call pushes
            w->asleep.store(1, std::memory_order_seq_cst);
            if (w->tail.load(std::memory_order_seq_cst) == h) w->cv.wait_for(lk, std::chrono::milliseconds(50));
            w->asleep.store(0, std::memory_order_seq_cst);
            spins = 0;
        }
        const Cmd c = w->ring[h % RING];
        int rc = 0;
        // a poisoned worker (the caller gave up on it and may have freed the list, its descriptors and streams) executes nothing:
        // it only consumes its ring
        if (!w->poisoned.load(std::memory_order_acquire)) {
            switch (c.kind) {
            case 0: rc = call(ops[c.idx], (void*)stream); break;
            case 1: rc = (int)hipStreamWaitEvent(stream, c.ev, 0); break;
            case 2: rc = (int)hipEventRecord(c.ev, stream); break;
            case 3: rc = (int)hipSetDevice(c.idx); ops = c.ops; stream = c.stream; break;
            }
        }
        if (c.kind == 1 || c.kind == 2) w->ev_used.fetch_add(1, std::memory_order_release);
        if (rc && !w->err.load()) w->err.store(rc);
        w->head.store(h + 1, std::memory_order_release);
    }
}

Worker* worker_for(int dev, int lane) {
    std::lock_guard<std::mutex> lk(g_workers_mutex);
    Worker*& slot = g_workers[dev][lane];
    if (!slot || slot->poisoned.load()) {
        Worker* w = new Worker();                                  // never freed: the thread outlives every static destructor
        std::thread(worker_main, w).detach();
        slot = w;                                                  // (a poisoned worker is abandoned with its thread)
    }
    return slot;
}

int push(Worker* w, const Cmd& c) {
    const unsigned t = w->tail.load(std::memory_order_relaxed);
    int spins = 0;
    while (t - w->head.load(std::memory_order_acquire) >= RING) {   // ring full: the worker is behind
        if (++spins > 200000000) { w->poisoned.store(1, std::memory_order_release); return -2; }
        __builtin_ia32_pause();
    }
    w->ring[t % RING] = c;
    w->tail.store(t + 1, std::memory_order_seq_cst);
    if (w->asleep.load(std::memory_order_seq_cst)) {
        std::lock_guard<std::mutex> lk(w->m);
        w->cv.notify_one();
    }
    return 0;
}

// the next event of the worker's pool, once the worker has executed the command that used the slot the last time round
int worker_event(Worker* w, hipEvent_t* out) {
    if (!w->ev_ready) {
        for (unsigned i = 0; i < EV_POOL; ++i) RD_CHECK(hipEventCreateWithFlags(&w->evpool[i], hipEventDisableTiming));
        w->ev_ready = true;
    }
    const auto t0 = std::chrono::steady_clock::now();
    int spins = 0;
    while (w->ev_issued - w->ev_used.load(std::memory_order_acquire) >= EV_POOL) {
        __builtin_ia32_pause();
        if ((++spins & 0xfffff) == 0 && std::chrono::steady_clock::now() - t0 > std::chrono::seconds(30)) {
            w->poisoned.store(1, std::memory_order_release);
            return -2;
        }
    }
    *out = w->evpool[w->ev_issued % EV_POOL];
    ++w->ev_issued;
    return 0;
}

// wait until the worker has executed everything pushed so far (bounded: a stuck runtime call must not hang the caller for ever; the
// worker is poisoned then -- it still holds commands that point into the caller's list)
int drain(Worker* w) {
    const unsigned t = w->tail.load(std::memory_order_relaxed);
    const auto t0 = std::chrono::steady_clock::now();
    int spins = 0;
    while ((int)(w->head.load(std::memory_order_acquire) - t) < 0) {
        __builtin_ia32_pause();
        if ((++spins & 0xfffff) == 0 && std::chrono::steady_clock::now() - t0 > std::chrono::seconds(30)) {
            w->poisoned.store(1, std::memory_order_release);
            return -2;
        }
    }
    return w->err.exchange(0);
}

// ------------------------------------------------------------------------------------------------ the walk
// Does an entry that makes a lane wait for the main stream follow entry i before the main stream is given anything else?  Then a launch
// on the main stream at i can carry the event of that fork on its own dispatch packet (common.h rd_launch) and the fork needs no record.
bool lane_edge_follows(const rd_launch_t* ops, int n, int i) {
    for (int j = i + 1; j < n; ++j) {
        const rd_launch_t& q = ops[j];
        if (q.op == RD_OP_FORK) {
            if (q.lane > 0) return true;
            continue;
        }
        if (q.op == RD_OP_JOIN || q.lane == 0) return false;    // the main stream's position changes first
        if (q.wait_main) return true;
    }
    return false;
}

// THE interpretation of a list (include/ramdsir.h): entries in order, malformed ones refused, the open-lane mask carried in and out;
// FORK / JOIN of lane 0 are ignored, a wait_main entry forks its lane first, a JOIN of a lane that is not open does nothing.  What a
// step DOES is the executor's: x.fork(lane) makes streams[lane] wait for the main stream's current position, x.join(lane) makes the
// main stream wait for streams[lane], x.launch(i, follows) launches entry i on its stream (follows(): lane_edge_follows, if asked).
template <class X> int walk(const rd_launch_t* ops, int n, int n_streams, uint32_t* open_lanes, int* bad_index, X& x) {
    uint32_t open = open_lanes ? *open_lanes : 0u;
    int rc = 0, i = 0;
    for (; i < n; ++i) {
        const rd_launch_t& o = ops[i];
        if (o.lane < 0 || o.lane >= n_streams || o.nargs < 0 || o.nargs > RD_LAUNCH_MAX_ARGS) { rc = -1; break; }
        const uint32_t bit = 1u << o.lane;
        if (o.op == RD_OP_FORK || o.op == RD_OP_JOIN) {
            if (o.lane == 0 || (o.op == RD_OP_JOIN && !(open & bit))) continue;
            open = o.op == RD_OP_FORK ? open | bit : open & ~bit;
            rc = o.op == RD_OP_FORK ? x.fork(o.lane) : x.join(o.lane);
        } else {
            if (o.lane > 0 && o.wait_main) { open |= bit; rc = x.fork(o.lane); }
            if (!rc) rc = x.launch(i, [&] { return lane_edge_follows(ops, n, i); });
        }
        if (rc) break;
    }
    if (rc && bad_index) *bad_index = i;
    if (open_lanes) *open_lanes = open;
    return rc;
}

// ---- executor 1: everything from the calling thread.  at_main: an event bound to the LAST launch of the main stream (its dispatch
// packet's completion), valid until the main stream is given anything else: forks at this position wait for it instead of recording
// one.  `bind` is off under stream capture (a captured graph takes its edges from recorded events) and with one stream.
struct Direct {
    const rd_launch_t* ops;
    void* const* streams;
    hipStream_t main_s;
    bool bind;
    hipEvent_t at_main = nullptr;
    int fork(int lane) {
        hipStream_t to = (hipStream_t)streams[lane];
        if (to == main_s) return 0;
        (at_main ? g_forks_bound : g_forks_recorded).fetch_add(1, std::memory_order_relaxed);
        return at_main ? (int)hipStreamWaitEvent(to, at_main, 0) : edge(main_s, to);
    }
    int join(int lane) {
        if ((hipStream_t)streams[lane] != main_s) at_main = nullptr;    // the main stream now also waits for the lane
        return edge((hipStream_t)streams[lane], main_s);
    }
    template <class F> int launch(int i, F follows) {
        void* st = streams[ops[i].lane];
        if ((hipStream_t)st != main_s) return call(ops[i], st);
        at_main = nullptr;
        hipEvent_t e;
        if (!(bind && follows() && next_event(&e) == 0)) return call(ops[i], st);
        rd_tls_stop_event = e;                                           // to the launch's (last) kernel: common.h rd_launch
        rd_tls_stop_used = 0;
        const int rc = call(ops[i], st);
        rd_tls_stop_event = nullptr;
        if (rd_tls_stop_used) at_main = e;                               // (rd_zero's fallback to the runtime's fills launches no kernel: the fork records)
        return rc;
    }
};

// ---- executor 2: feeds the lane worker threads (above); lane 0's entries are launched by the caller.  A worker's error surfaces at
// the lane's join, or in finish() with bad_index -1.
struct Threaded {
    const rd_launch_t* ops;
    void* const* streams;
    hipStream_t main_s;
    int dev;
    Worker* ws[32] = {};
    int main_launch_rc = 0;
    Worker* lane_worker(int lane) {
        if (!ws[lane]) {
            ws[lane] = worker_for(dev, lane);
            Cmd c{3, dev, nullptr, ops, (hipStream_t)streams[lane]};
            if (push(ws[lane], c)) return nullptr;
        }
        return ws[lane];
    }
    int fork(int lane) {
        Worker* w = lane_worker(lane);
        if (!w) return -2;
        if ((hipStream_t)streams[lane] == main_s) return 0;
        hipEvent_t e;
        if (const int err = worker_event(w, &e)) return err;
        RD_CHECK(hipEventRecord(e, main_s));
        return push(w, Cmd{1, 0, e, nullptr, nullptr});
    }
    int join(int lane) {
        Worker* w = lane_worker(lane);
        if (!w) return -2;
        if ((hipStream_t)streams[lane] == main_s) return drain(w);
        hipEvent_t e;
        int rc = worker_event(w, &e);
        if (!rc) rc = push(w, Cmd{2, 0, e, nullptr, nullptr});
        if (!rc) rc = drain(w);                                    // the record has been enqueued (and everything before it)
        return rc ? rc : (int)hipStreamWaitEvent(main_s, e, 0);
    }
    template <class F> int launch(int i, F) {
        if (ops[i].lane == 0) return main_launch_rc = call(ops[i], (void*)main_s);
        Worker* w = lane_worker(ops[i].lane);
        return w ? push(w, Cmd{0, i, nullptr, nullptr, nullptr}) : -2;
    }
    // every worker has enqueued what it was given (descriptors may be changed by the caller afterwards)
    int finish(int rc, int n_streams, int* bad_index) {
        if (main_launch_rc && bad_index) ++*bad_index;             // (this walk has always named the entry BEHIND a failing main-lane launch)
        for (int k = 1; k < n_streams; ++k)
            if (ws[k]) {
                const int e = drain(ws[k]);
                if (e && !rc) { rc = e; if (bad_index) *bad_index = -1; }
            }
        return rc;
    }
};

// ---- executor 3: launches nothing and writes the steps out (rd_run_list_schedule).  Lanes are taken as distinct streams.
struct Recorder {
    const rd_launch_t* ops;
    rd_step_t* steps;
    int n = 0;
    int add(int kind, int lane, int index, int carries) { steps[n++] = rd_step_t{kind, lane, index, carries}; return 0; }
    int fork(int lane) { return add(RD_STEP_FORK, lane, -1, 0); }
    int join(int lane) { return add(RD_STEP_JOIN, lane, -1, 0); }
    template <class F> int launch(int i, F follows) { return row_of(ops[i]) ? add(RD_STEP_LAUNCH, ops[i].lane, i, ops[i].lane == 0 && follows()) : -1; }
};

}  // namespace

extern "C" int rd_op_code(const char* entry_point) {
    for (int k = 0; entry_point && k < RD_OP_END_ - RD_OP_CONV; ++k)
        if (!strcmp(entry_point, OPS[k].name)) return RD_OP_CONV + k;
    return -1;
}

extern "C" int rd_run_list_schedule(const rd_launch_t* ops, int n, int n_streams, uint32_t* open_lanes, int* bad_index, rd_step_t* steps, int* n_steps) {
    if (n_streams < 1 || n_streams > 32 || n < 0 || !n_steps || (n > 0 && (!ops || !steps))) return -1;
    Recorder x{ops, steps};
    const int rc = walk(ops, n, n_streams, open_lanes, bad_index, x);
    *n_steps = x.n;
    return rc;
}

// which main-lane entries of a list would carry a fork's event on their own dispatch packet: the schedule's `carries`, by entry
extern "C" int rd_run_list_fork_plan(const rd_launch_t* ops, int n, unsigned char* carries) {
    if (n < 0 || (n > 0 && (!ops || !carries))) return -1;
    memset(carries, 0, (size_t)n);
    std::vector<rd_step_t> steps(2 * (size_t)n);
    int n_steps = 0;
    (void)rd_run_list_schedule(ops, n, 32, nullptr, nullptr, steps.data(), &n_steps);
    for (int k = 0; k < n_steps; ++k)
        if (steps[k].kind == RD_STEP_LAUNCH) carries[steps[k].index] = (unsigned char)steps[k].carries;
    return 0;
}

extern "C" void rd_run_list_fork_counts(long long* bound, long long* recorded) {
    if (bound) *bound = g_forks_bound.load();
    if (recorded) *recorded = g_forks_recorded.load();
}

extern "C" int rd_run_list_bind_fork_events(int enable) { return g_bind_fork_events.exchange(enable ? 1 : 0); }

extern "C" int rd_run_list_threads(int enable) { return g_threads_enabled.exchange(enable ? 1 : 0); }

extern "C" int rd_join_lanes(void* const* streams, int n_streams, uint32_t mask) {
    for (int k = 1; k < n_streams && k < 32; ++k)
        if (mask & (1u << k)) {
            const int err = edge((hipStream_t)streams[k], (hipStream_t)streams[0]);
            if (err) return err;
        }
    return 0;
}

extern "C" int rd_run_list(const rd_launch_t* ops, int n, void* const* streams, int n_streams, uint32_t* open_lanes, int* bad_index) {
    if (n_streams < 1 || n_streams > 32) return -1;
    hipStream_t main_s = (hipStream_t)streams[0];
    // worker threads and bound fork events only with side streams and outside stream capture (a capture is recorded by the capturing
    // thread, from recorded events)
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    const bool eager = n_streams > 1 && hipStreamIsCapturing(main_s, &cap) == hipSuccess && cap == hipStreamCaptureStatusNone;
    if (eager && g_threads_enabled.load()) {
        int dev = 0;
        RD_CHECK(hipGetDevice(&dev));
        if (dev < 0 || dev >= EV_MAX_DEV) return -1;
        Threaded x{ops, streams, main_s, dev};
        return x.finish(walk(ops, n, n_streams, open_lanes, bad_index, x), n_streams, bad_index);
    }
    Direct x{ops, streams, main_s, eager && g_bind_fork_events.load() != 0};
    return walk(ops, n, n_streams, open_lanes, bad_index, x);
}
