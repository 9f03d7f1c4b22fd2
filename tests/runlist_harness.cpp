// Stand-alone trace harness of the launch list (csrc/runlist.hip), for a machine without a GPU: helper of test_cpu_runlist.py.
//
// It links runlist's object (compiled with --offload-host-only) against the fakes below -- the seven HIP calls runlist.hip makes and the
// 24 entry points a list can hold -- and uses the public ABI of include/ramdsir.h only (plus common.h's two thread-local variables of
// rd_launch), so it links unchanged against an older runlist.hip.  For every case it prints one line of JSON: return code, bad_index,
// open mask, the bound / recorded fork counts, and per stream the ordered operations:
//   "rd_x(...) ev=E t=T"  a launch with every argument as the stub received it, in its own type (p: pointer, i: int, l: int64_t,
//                         f: the bits of a float); E = none | took | declined: the list offered a fork's event to the launch
//                         (rd_tls_stop_event) and the launch bound it (rd_launch does) or not (rd_zero's fallback to the runtime's
//                         fills); T = c | w: issued by the calling thread or by a lane worker thread;
//   "wait sK#N via=V t=T" a hipStreamWaitEvent, resolved to stream K's operation number N (-1: nothing was enqueued there) and to
//                         how the event got there (V = record | bound), never to an event handle.
// A stream is named by the lowest index of streams[] that holds its handle.  Per stream the order is deterministic with the worker
// threads on as well (one producer per stream); a lane whose stream aliases the main stream would have two, so that list runs with the
// threads off.  `runlist_harness schedule` prints, for the lists without aliases, rd_run_list_schedule's steps, rd_run_list_fork_plan's
// flags and the single-threaded walk's operations in the order they were issued, in the schedule's words.
#include <hip/hip_runtime_api.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <map>
#include <mutex>
#include <string>
#include <thread>
#include <vector>
#include "ramdsir.h"

extern thread_local hipEvent_t rd_tls_stop_event;
extern thread_local int rd_tls_stop_used;
extern "C" int rd_run_list_schedule(const rd_launch_t*, int, int, uint32_t*, int*, rd_step_t*, int*) __attribute__((weak));

namespace {

constexpr uint64_t FAIL = 0xBAD00000000ull;       // first argument of a launch that returns 77
constexpr int DECLINE = -99;                      // rd_zero's n: the launch binds no event

struct Ev { int stream = -1, idx = -1; bool bound = false, set = false; };
std::mutex g_m;
std::thread::id g_caller;
std::vector<void*> g_streams;                     // this case's streams[]
std::map<int, std::vector<std::string>> g_ops;    // per stream
std::vector<std::string> g_order;                 // schedule mode: every operation in issue order, in the schedule's words
const rd_launch_t* g_list = nullptr;
int g_list_n = 0, g_next_launch = 0;
bool g_capture = false;

int stream_name(const void* s) {
    for (size_t k = 0; k < g_streams.size(); ++k)
        if (g_streams[k] == s) return (int)k;
    return 99;
}
char thread_tag() { return std::this_thread::get_id() == g_caller ? 'c' : 'w'; }

void fmt(std::string& s, const void* v) { char b[32]; snprintf(b, sizeof b, "p:%#llx", (unsigned long long)(uintptr_t)v); s += b; }
void fmt(std::string& s, int v) { char b[32]; snprintf(b, sizeof b, "i:%d", v); s += b; }
void fmt(std::string& s, int64_t v) { char b[32]; snprintf(b, sizeof b, "l:%lld", (long long)v); s += b; }
void fmt(std::string& s, float v) { uint32_t u; memcpy(&u, &v, 4); char b[32]; snprintf(b, sizeof b, "f:%#010x", u); s += b; }

template <class First, class... A> int launch(const char* name, void* stream, bool decline, First first, A... rest) {
    std::lock_guard<std::mutex> lk(g_m);
    std::string s = std::string(name) + "(";
    fmt(s, first);
    ((s += ", ", fmt(s, rest)), ...);
    const int st = stream_name(stream);
    const char* ev = "none";
    if (rd_tls_stop_event) {
        ev = decline ? "declined" : "took";
        if (!decline) {
            rd_tls_stop_used = 1;
            Ev* e = (Ev*)rd_tls_stop_event;
            *e = Ev{st, (int)g_ops[st].size(), true, true};
        }
    }
    s += std::string(") ev=") + ev + " t=" + thread_tag();
    g_ops[st].push_back(s);
    while (g_next_launch < g_list_n && (g_list[g_next_launch].op == RD_OP_FORK || g_list[g_next_launch].op == RD_OP_JOIN)) ++g_next_launch;
    if (g_next_launch < g_list_n) {
        char b[64];
        snprintf(b, sizeof b, "launch %d lane %d carries %d", g_next_launch, g_list[g_next_launch].lane, rd_tls_stop_event ? 1 : 0);
        g_order.push_back(b);
        ++g_next_launch;
    }
    return (uint64_t)(uintptr_t)first == FAIL ? 77 : 0;
}

}  // namespace

// ------------------------------------------------------------------------------------------------ the seven HIP calls
hipError_t hipGetDevice(int* d) { *d = 0; return hipSuccess; }
hipError_t hipSetDevice(int) { return hipSuccess; }
hipError_t hipEventCreateWithFlags(hipEvent_t* e, unsigned) { *e = (hipEvent_t) new Ev(); return hipSuccess; }
hipError_t hipEventRecord(hipEvent_t e, hipStream_t s) {
    std::lock_guard<std::mutex> lk(g_m);
    const int st = stream_name(s);
    *(Ev*)e = Ev{st, (int)g_ops[st].size() - 1, false, true};
    return hipSuccess;
}
hipError_t hipStreamWaitEvent(hipStream_t s, hipEvent_t e, unsigned) {
    std::lock_guard<std::mutex> lk(g_m);
    const Ev& v = *(Ev*)e;
    const int st = stream_name(s);
    char b[96];
    if (!v.set) snprintf(b, sizeof b, "wait unrecorded t=%c", thread_tag());
    else snprintf(b, sizeof b, "wait s%d#%d via=%s t=%c", v.stream, v.idx, v.bound ? "bound" : "record", thread_tag());
    g_ops[st].push_back(b);
    snprintf(b, sizeof b, st == 0 ? "join %d" : "fork %d", st == 0 ? v.stream : st);
    g_order.push_back(b);
    return hipSuccess;
}
hipError_t hipStreamIsCapturing(hipStream_t, hipStreamCaptureStatus* st) {
    *st = g_capture ? hipStreamCaptureStatusActive : hipStreamCaptureStatusNone;
    return hipSuccess;
}
const char* hipGetErrorString(hipError_t) { return "fake"; }

// ------------------------------------------------------------------------------------------------ the 24 entry points
extern "C" {
int rd_conv(const rd_conv_t* p, int dtype, void* st) { return launch("rd_conv", st, false, (const void*)p, dtype); }
int rd_wgrad(const rd_wgrad_t* p, int dtype, void* st) { return launch("rd_wgrad", st, false, (const void*)p, dtype); }
int rd_conv_bwd_fused(const rd_conv_t* d, const rd_wgrad_t* w, int dtype, void* st) {
    return launch("rd_conv_bwd_fused", st, false, (const void*)d, (const void*)w, dtype);
}
int rd_conv_bwd_fused_reduce(const rd_conv_t* d, const rd_wgrad_t* w, int dtype, void* st) {
    return launch("rd_conv_bwd_fused_reduce", st, false, (const void*)d, (const void*)w, dtype);
}
int rd_pack_weights_batched(const float* params, void* packed, const rd_pack_entry_t* table, int n, int64_t total, int dtype, void* st) {
    return launch("rd_pack_weights_batched", st, false, (const void*)params, (const void*)packed, (const void*)table, n, total, dtype);
}
int rd_bn_finalize_fwd(const rd_bn_fwd_t* p, void* st) { return launch("rd_bn_finalize_fwd", st, false, (const void*)p); }
int rd_bn_finalize_bwd(const rd_bn_bwd_t* p, void* st) { return launch("rd_bn_finalize_bwd", st, false, (const void*)p); }
int rd_gn_finalize_fwd(const rd_bn_fwd_t* p, void* st) { return launch("rd_gn_finalize_fwd", st, false, (const void*)p); }
int rd_gn_finalize_bwd(const rd_bn_bwd_t* p, void* st) { return launch("rd_gn_finalize_bwd", st, false, (const void*)p); }
int rd_up_stats(const void* t, double* stats, void* y, int N, int h, int w, int C, int G, const int32_t* gs, int dtype, int slots, void* st) {
    return launch("rd_up_stats", st, false, t, (const void*)stats, (const void*)y, N, h, w, C, G, (const void*)gs, dtype, slots);
}
int rd_bn_stats(const void* x, double* stats, int N, int H, int W, int C, int G, const int32_t* gs, int dtype, void* st) {
    return launch("rd_bn_stats", st, false, x, (const void*)stats, N, H, W, C, G, (const void*)gs, dtype);
}
int rd_up_bwd(const void* g, const void* t, void* dt, const float* P, const float* Q, const float* R, int N, int h, int w, int C, int G,
              const int32_t* gs, int dtype, const rd_bn_bwd_t* fin, int fin_flags, void* st) {
    return launch("rd_up_bwd", st, false, g, t, (const void*)dt, (const void*)P, (const void*)Q, (const void*)R, N, h, w, C, G, (const void*)gs,
                  dtype, (const void*)fin, fin_flags);
}
int rd_pool_fwd(const void* z, const float* scale, const float* shift, float slope, void* out, int N, int Ho, int Wo, int C, int G,
                const int32_t* gs, int dtype, const rd_bn_fwd_t* fin, int fin_flags, void* st) {
    return launch("rd_pool_fwd", st, false, z, (const void*)scale, (const void*)shift, slope, (const void*)out, N, Ho, Wo, C, G, (const void*)gs,
                  dtype, (const void*)fin, fin_flags);
}
int rd_pool_bwd(const void* gp, const void* z, const float* scale, const float* shift, float slope, int act, void* g, int accumulate,
                double* bstats, int N, int Ho, int Wo, int C, int G, const int32_t* gs, int dtype, int slots, void* st) {
    return launch("rd_pool_bwd", st, false, gp, z, (const void*)scale, (const void*)shift, slope, act, (const void*)g, accumulate,
                  (const void*)bstats, N, Ho, Wo, C, G, (const void*)gs, dtype, slots);
}
int rd_bn_apply(const void* x, const void* x2, void* out, const float* a, const float* b, const float* c, float slope, int N, int H, int W,
                int C, int G, const int32_t* gs, int dtype, void* st) {
    return launch("rd_bn_apply", st, false, x, x2, (const void*)out, (const void*)a, (const void*)b, (const void*)c, slope, N, H, W, C, G,
                  (const void*)gs, dtype);
}
int rd_nchw_to_nhwc(const float* x, void* y, int N, int C, int H, int W, int cstride, int dtype, void* st) {
    return launch("rd_nchw_to_nhwc", st, false, (const void*)x, (const void*)y, N, C, H, W, cstride, dtype);
}
int rd_nhwc_to_nchw(const void* z, float* y, const float* scale, const float* shift, int act, float slope, int N, int C, int H, int W, int G,
                    const int32_t* gs, int dtype, void* st) {
    return launch("rd_nhwc_to_nchw", st, false, z, (const void*)y, (const void*)scale, (const void*)shift, act, slope, N, C, H, W, G,
                  (const void*)gs, dtype);
}
int rd_grad_in(const float* dy, const void* z, void* g, const float* scale, const float* shift, double* bstats, int act, float slope,
               int accumulate, int N, int C, int H, int W, int G, const int32_t* gs, int dtype, void* st) {
    return launch("rd_grad_in", st, false, (const void*)dy, z, (const void*)g, (const void*)scale, (const void*)shift, (const void*)bstats, act,
                  slope, accumulate, N, C, H, W, G, (const void*)gs, dtype);
}
int rd_colsum(const void* x, float* out, float* ws, int64_t npix, int C, int cstride, float beta, int dtype, void* st) {
    return launch("rd_colsum", st, false, x, (const void*)out, (const void*)ws, npix, C, cstride, beta, dtype);
}
int rd_seg_loss(const rd_seg_loss_t* p, int dtype, void* st) { return launch("rd_seg_loss", st, false, (const void*)p, dtype); }
int rd_rec_loss(const void* logits, const void* target, void* dlogits, float* mse, float* ws, int B, int H, int W, int C, int tcs, int dcs,
                int G, const int32_t* gs, float lambda_rec, int dtype, void* st) {
    return launch("rd_rec_loss", st, false, logits, target, (const void*)dlogits, (const void*)mse, (const void*)ws, B, H, W, C, tcs, dcs, G,
                  (const void*)gs, lambda_rec, dtype);
}
int rd_adam_step(const rd_adam_t* p, void* st) { return launch("rd_adam_step", st, false, (const void*)p); }
int rd_zero(void* const* ptrs, const int64_t* bytes, int n, void* st) {
    return launch("rd_zero", st, n == DECLINE, (const void*)ptrs, (const void*)bytes, n);
}
int rd_ram_mix(const rd_ram_t* p, int dtype, void* st) { return launch("rd_ram_mix", st, false, (const void*)p, dtype); }
}

// ------------------------------------------------------------------------------------------------ lists
namespace {

using List = std::vector<rd_launch_t>;

rd_launch_t entry(int op, int lane, int wait_main, std::vector<uint64_t> a = {}) {
    rd_launch_t e;
    memset(&e, 0, sizeof e);
    e.op = op, e.lane = lane, e.wait_main = wait_main, e.nargs = (int)a.size();
    for (size_t i = 0; i < a.size() && i < RD_LAUNCH_MAX_ARGS; ++i) e.a[i] = a[i];
    return e;
}
uint64_t fbits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
rd_launch_t conv(uint64_t tag, int lane = 0, int wait_main = 0) { return entry(RD_OP_CONV, lane, wait_main, {0x7f0000001000ull + tag, 1}); }
rd_launch_t wgrad(uint64_t tag, int lane, int wait_main) { return entry(RD_OP_WGRAD, lane, wait_main, {0x7f0000002000ull + tag, 1}); }
rd_launch_t adam(int lane = 0) { return entry(RD_OP_ADAM_STEP, lane, 0, {0x7f0000003000ull}); }
rd_launch_t zero(int n, int lane = 0) { return entry(RD_OP_ZERO, lane, 0, {0x7f0000004000ull, 0x7f0000004800ull, (uint64_t)(int64_t)n}); }
rd_launch_t fork(int lane) { return entry(RD_OP_FORK, lane, 0); }
rd_launch_t join(int lane) { return entry(RD_OP_JOIN, lane, 0); }

// slot s of op `op`: a pointer above 2^32, an int64_t above 2^32, and in the low word a negative int (odd slots), a NaN (every fourth) or a
// denormal: whatever type the slot has, the value is distinct and uncommon; every fifth slot is 0 (a null pointer)
uint64_t slot_value(int op, int s) {
    if (s % 5 == 4) return 0;
    const uint64_t low = (s % 4 == 3 ? 0x7fc00000u : s % 2 ? 0x80000000u : 0u) | (uint32_t)op << 12 | (uint32_t)s << 4 | 0xbu;
    return (uint64_t)(0x7000 + op) << 32 | low;
}
const int ARITY[24] = {2, 2, 3, 3, 6, 1, 1, 1, 1, 11, 9, 15, 14, 17, 14, 8, 13, 16, 8, 2, 15, 1, 3, 2};      // RD_OP_CONV ... RD_OP_RAM_MIX
rd_launch_t any_op(int op, int lane, int wait_main, int dn = 0) {
    std::vector<uint64_t> a;
    for (int s = 0; s < ARITY[op - 10] + dn; ++s) a.push_back(slot_value(op, s));
    return entry(op, lane, wait_main, a);
}

void* stream_handle(int k) { return (void*)(uintptr_t)(0x51000000ull + 0x100 * k); }

void print_strings(const std::vector<std::string>& v) {
    printf("[");
    for (size_t i = 0; i < v.size(); ++i) printf("%s\"%s\"", i ? ", " : "", v[i].c_str());
    printf("]");
}

bool g_first = true;
void begin_case(const std::string& name, const List& l, const std::vector<void*>& streams) {
    g_streams = streams;
    g_ops.clear();
    g_order.clear();
    g_list = l.data(), g_list_n = (int)l.size(), g_next_launch = 0;
    printf("%s\"%s\": {", g_first ? "" : ",\n", name.c_str());
    g_first = false;
}
void print_streams() {
    printf("\"streams\": {");
    bool first = true;
    for (auto& kv : g_ops) {
        printf("%s\"%d\": ", first ? "" : ", ", kv.first);
        print_strings(kv.second);
        first = false;
    }
    printf("}}");
}

struct Run { bool bind, threads, capture; };

void run_case(const std::string& name, const List& l, int n_streams, Run r, uint32_t open_in = 0, int alias = -1, bool null_out = false) {
    std::vector<void*> streams;
    for (int k = 0; k < (n_streams > 0 ? n_streams : 1); ++k) streams.push_back(k == alias ? stream_handle(0) : stream_handle(k));
    char sw[16];
    snprintf(sw, sizeof sw, "/b%dt%dc%d", r.bind, r.threads, r.capture);
    begin_case(name + sw, l, streams);
    rd_run_list_bind_fork_events(r.bind);
    rd_run_list_threads(r.threads);
    g_capture = r.capture;
    long long b0, r0, b1, r1;
    rd_run_list_fork_counts(&b0, &r0);
    uint32_t open = open_in;
    int bad = -7;
    const int rc = rd_run_list(l.data(), (int)l.size(), streams.data(), n_streams, null_out ? nullptr : &open, null_out ? nullptr : &bad);
    rd_run_list_fork_counts(&b1, &r1);
    printf("\"rc\": %d, \"bad\": %d, \"open\": %u, \"forks\": [%lld, %lld], ", rc, bad, open, b1 - b0, r1 - r0);
    print_streams();
}

void all_switches(const std::string& name, const List& l, int n_streams, uint32_t open_in = 0) {
    for (int b = 1; b >= 0; --b)
        for (int t = 0; t < 2; ++t)
            for (int c = 0; c < 2; ++c) run_case(name, l, n_streams, Run{b != 0, t != 0, c != 0}, open_in);
}

struct Named { std::string name; List l; int n_streams; uint32_t open_in; };

std::vector<Named> lists() {
    std::vector<Named> v;
    // the two lists of test_launch_list_packing_and_lanes (lanes: 1 = side0, 2 = rec)
    v.push_back({"packing1", {conv(0), fork(2),
                              entry(RD_OP_POOL_FWD, 2, 0, {0x1000, 0, 0, fbits(0.25f), 0x2000, 4, 5, 6, 16, 2, 0x7f0000005000ull, 1, 0, 0}),
                              wgrad(0, 1, 1), join(2), adam()}, 3, 0});
    v.push_back({"packing2", {conv(0), conv(1), wgrad(0, 1, 1), wgrad(1, 1, 1), conv(2), join(1), wgrad(2, 1, 1), adam()}, 3, 0});
    List all;
    for (int op = RD_OP_CONV; op <= RD_OP_RAM_MIX; ++op) all.push_back(any_op(op, (op - 10) % 3, (op - 10) % 3 ? 1 : 0));
    v.push_back({"every_op", all, 3, 0});
    v.push_back({"fork_join_lane0", {conv(0), fork(0), join(0), conv(1), fork(0), wgrad(0, 1, 1), conv(2), join(0), fork(2), conv(3, 2), join(1), join(2)}, 3, 0});
    v.push_back({"join_of_closed_lane", {conv(0), join(1), conv(1), fork(1), wgrad(0, 1, 0), join(1), join(1), adam()}, 3, 0});
    v.push_back({"open_on_entry", {conv(0), join(2), wgrad(0, 1, 1), conv(1, 2), adam()}, 3, 0x6});
    v.push_back({"wait_main_back_to_back", {conv(0), wgrad(0, 1, 1), wgrad(1, 2, 1), wgrad(2, 1, 1), conv(1), fork(1), fork(2), conv(2, 2), adam(),
                                            wgrad(3, 2, 1), join(1), join(2)}, 3, 0});
    v.push_back({"zero_declines", {zero(DECLINE), fork(1), wgrad(0, 1, 0), zero(3), wgrad(1, 2, 1), zero(DECLINE), wgrad(2, 2, 1), join(1), join(2)}, 3, 0});
    List em = {conv(0), wgrad(0, 1, 1), conv(1), wgrad(1, 1, 1), adam(), join(1)};
    em[2].a[0] = FAIL;
    v.push_back({"error_on_main_lane", em, 3, 0});
    List es = {conv(0), wgrad(0, 1, 1), wgrad(1, 1, 1), conv(1), wgrad(2, 2, 1), join(1), adam()};
    es[2].a[0] = FAIL;
    v.push_back({"error_on_side_lane", es, 3, 0});
    v.push_back({"lane_beyond_streams", {conv(0), wgrad(0, 1, 1), wgrad(1, 3, 1), conv(1)}, 3, 0});
    v.push_back({"negative_lane", {conv(0), fork(-1), conv(1)}, 3, 0});
    v.push_back({"unknown_op", {conv(0), entry(34, 0, 0, {1, 2}), conv(1)}, 3, 0});
    v.push_back({"unknown_op_on_lane", {conv(0), entry(9, 1, 1, {1, 2}), conv(1)}, 3, 0});
    v.push_back({"op_zero", {conv(0), entry(0, 0, 0), conv(1)}, 3, 0});
    v.push_back({"nargs_19", {conv(0), entry(RD_OP_POOL_BWD, 0, 0, std::vector<uint64_t>(19, 5)), conv(1)}, 3, 0});
    v.push_back({"nargs_negative", {conv(0), entry(RD_OP_FORK, 1, 0), conv(1)}, 3, 0});
    v.back().l[1].nargs = -1;
    for (int op : {(int)RD_OP_ADAM_STEP, (int)RD_OP_COLSUM, (int)RD_OP_POOL_BWD})
        for (int dn : {-1, 1}) {
            v.push_back({"nargs_op" + std::to_string(op) + (dn < 0 ? "_short" : "_over"), {conv(0), wgrad(0, 1, 1), any_op(op, op == RD_OP_COLSUM ? 1 : 0, 0, dn), conv(1)}, 3, 0});
        }
    v.push_back({"empty", {}, 3, 0x2});
    return v;
}

}  // namespace

int main(int argc, char** argv) {
    g_caller = std::this_thread::get_id();
    const bool schedule = argc > 1 && !strcmp(argv[1], "schedule");
    printf("{\n");
    if (schedule) {
        if (!rd_run_list_schedule) { fprintf(stderr, "this runlist has no rd_run_list_schedule\n"); return 2; }
        for (const Named& c : lists()) {
            const List& l = c.l;
            std::vector<void*> streams;
            for (int k = 0; k < c.n_streams; ++k) streams.push_back(stream_handle(k));
            begin_case(c.name, l, streams);
            std::vector<rd_step_t> steps(2 * l.size() + 1);
            std::vector<unsigned char> plan(l.size() + 1);
            uint32_t open = c.open_in;
            int bad = -7, n_steps = -7;
            int rc = rd_run_list_schedule(l.data(), (int)l.size(), c.n_streams, &open, &bad, steps.data(), &n_steps);
            printf("\"rc\": %d, \"bad\": %d, \"open\": %u, \"steps\": ", rc, bad, open);
            std::vector<std::string> s;
            for (int i = 0; i < n_steps; ++i) {
                char b[64];
                if (steps[i].kind == RD_STEP_LAUNCH) snprintf(b, sizeof b, "launch %d lane %d carries %d", steps[i].index, steps[i].lane, steps[i].carries);
                else snprintf(b, sizeof b, "%s %d", steps[i].kind == RD_STEP_FORK ? "fork" : "join", steps[i].lane);
                s.push_back(b);
            }
            print_strings(s);
            rc = rd_run_list_fork_plan(l.data(), (int)l.size(), plan.data());
            printf(", \"plan_rc\": %d, \"plan\": [", rc);
            for (size_t i = 0; i < l.size(); ++i) printf("%s%d", i ? ", " : "", plan[i]);
            rd_run_list_bind_fork_events(1);
            rd_run_list_threads(0);
            g_capture = false;
            open = c.open_in, bad = -7;
            rc = rd_run_list(l.data(), (int)l.size(), streams.data(), c.n_streams, &open, &bad);
            printf("], \"direct_rc\": %d, \"direct_bad\": %d, \"direct_open\": %u, \"direct\": ", rc, bad, open);
            print_strings(g_order);
            printf("}");
        }
        printf("\n}\n");
        return 0;
    }
    for (const Named& c : lists()) all_switches(c.name, c.l, c.n_streams, c.open_in);
    // null open_lanes / bad_index
    const Named p1 = lists()[0];
    run_case("packing1_null_outputs", p1.l, 3, Run{true, false, false}, 0, -1, true);
    run_case("error_null_outputs", lists()[8].l, 3, Run{true, true, false}, 0, -1, true);
    // a lane whose stream handle is the main stream's (threads off: two producers on one stream have no order to pin)
    const List alias = {conv(0), fork(2), conv(1, 2), wgrad(0, 2, 1), conv(2), fork(1), conv(3, 2), wgrad(1, 1, 1), join(2), conv(4), wgrad(2, 1, 1),
                        join(1), adam()};
    for (int b = 1; b >= 0; --b)
        for (int c = 0; c < 2; ++c) run_case("lane_aliases_main", alias, 3, Run{b != 0, false, c != 0}, 0, 2);
    // n_streams 0, 1, 32, 33
    const List one = {conv(0), adam()};
    const List wide = {conv(0), wgrad(0, 31, 1), fork(5), conv(1, 5), join(31), adam()};
    for (int t = 0; t < 2; ++t) {
        run_case("n_streams_0", one, 0, Run{true, t != 0, false});
        run_case("n_streams_1", one, 1, Run{true, t != 0, false});
        run_case("n_streams_1_with_lane", p1.l, 1, Run{true, t != 0, false});
        run_case("n_streams_32", wide, 32, Run{true, t != 0, false});
        run_case("n_streams_33", wide, 33, Run{true, t != 0, false});
    }
    // rd_join_lanes: several mask bits, bit 0, a bit beyond the streams, an aliased lane
    for (int alias_lane : {-1, 2}) {
        std::vector<void*> streams;
        for (int k = 0; k < 5; ++k) streams.push_back(k == alias_lane ? stream_handle(0) : stream_handle(k));
        const List pre = {conv(0), conv(1, 1), conv(2, 2), conv(3, 4)};
        begin_case(alias_lane < 0 ? "join_lanes" : "join_lanes_alias", pre, streams);
        rd_run_list_threads(0);
        g_capture = false;
        int rc = rd_run_list(pre.data(), (int)pre.size(), streams.data(), 5, nullptr, nullptr);
        const int rc2 = rd_join_lanes(streams.data(), 5, 0x35u);          // lanes 0 (ignored), 2, 4, 5 (beyond)
        printf("\"rc\": %d, \"join_rc\": %d, ", rc, rc2);
        print_streams();
    }
    printf("\n}\n");
    return 0;
}
