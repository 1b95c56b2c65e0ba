// Native multi-GPU solver loop: one rank (process, GPU) per volume TILE -- a Px x Py x Pz grid of tiles (2 x 2 x 2 on 8 GPUs,
// BASELINE config 4; 1 x 1 x N = z-slabs).
//
// Every field of a rank is a local array = owned cells + 4 halo cells on each side that faces a neighbour.  One iteration needs
// ONE exchange (Option B): pass A produces nabla_U on the owned cells, the 4-cell faces (and the 4 x 4 edge strips:
// the one-cell shells below read nabla_U diagonally across a tile edge, never across a corner) travel to the 3 face + 3 edge
// neighbours of a 2 x 2 x 2 tile, and pass B then updates psi / phi_n o psi on owned +- 1 along each axis -- the radius-3
// convolution is exact there, so the values the next pass A reads are never exchanged.  phi_n is replicated.
//
// The exchange is PART OF PASS A's LAUNCH (solver_kernels.hip, tile_potential_gradient_kernel): the cells of every message
// are evaluated by "push boxes" -- numbered first; short marches for the y / z faces (which also store their cells at home: the
// owned block leaves them out), lane per cell for the x face and the edge strips -- that store straight into the destination.
// Transports:
//   DIRECT    the destination is the neighbour's own nabla_U array, peer-mapped over xGMI (hipIpc; sobfu_hip_tiled_connect).
//             No pack, no unpack, no communication launch: the last push workgroup raises this rank's arrival flag at its
//             neighbours, the last workgroup of the launch waits for theirs (with a deadline), so the transfers overlap the
//             owned block's compute inside ONE launch and an iteration is two launches, as on a single GPU.  nabla_U is
//             double-buffered by iteration parity: a neighbour's pass A of iteration k+1 stores into the half this rank's
//             pass B of iteration k does not read; its pass A of k+2 cannot start before this rank's flag of k+1, which this
//             rank raises after its pass B of k has retired.  The max-norm rows become global the same way (every rank stores
//             its row maximum into entry `rank` of that row at every other rank): no collective anywhere in the loop.
//   RCCL      the destination is the packed send buffer; one grouped ncclSend / ncclRecv per exchange and one scatter kernel
//             (z-slabs: whole planes in place, and the overlapped schedules of round 1).
//   CALLBACK  the same buffers handed to a user function (in-process loopback and gloo bring-up transports of the tests).
// The one-cell x / y shells of pass B are DIRECT boxes of its launch (lane per cell), the z shells extra planes of the march.
//
// Schedules of the RCCL z-slab path: serial (pass A, exchange, pass B in line), or overlapped as in tests/tiled_reference.py:
//     A_bnd (planes next to an interior face)  ->  event  ->  [comm stream] group{send, recv} of 4 nabla_U planes / face
//     A_int, B_int (planes whose +-3 taps are owned)            ... run while the exchange is in flight
//     wait(comm)  ->  B_bnd (remaining planes out to owned +-1)
// When a non-negative threshold can fire the device-side gate needs the GLOBAL max-norm: see tiled_begin for the ping-pong /
// late-gate scheme that keeps that reduction off the critical path.
//
// Reading order: the handle (members in release order) and its MaxNormRows; create3 / connect; the transports (transfer,
// exchange_*); the loop -- tiled_begin, LoopCtx, pass_a / pass_b, then one function per way of issuing an iteration (issue_tile,
// issue_slab_serial, issue_slab_overlapped: the schedules drawn above), tiled_step_impl dispatching to them, tiled_end.
//
// RCCL is not a link-time dependency: the host process (PyTorch) has already loaded librccl.so; sobfu_hip_tiled_load_rccl
// dlopen()s that same file and resolves the entry points used here, so libsobfu_hip.so still loads on a machine
// without RCCL and a process never holds two copies of the library.
#include <dlfcn.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <thread>
#include <vector>

#include "sobfu_device.hpp"
#include "sobfu_hip.h"
#include "sobfu_host.hpp"
#include "sobfu_launch.hpp"
#include "sobfu_tile_layout.hpp"

// The handful of RCCL (= NCCL API) types this file needs, declared here so that neither building nor loading the library
// depends on an RCCL installation (values as in rccl.h; the entry points are resolved with dlsym at run time).
extern "C" {
typedef struct ncclComm* ncclComm_t;
typedef struct { char internal[128]; } ncclUniqueId;
typedef enum { ncclSuccess = 0 } ncclResult_t;
typedef enum { ncclUint32 = 3, ncclFloat32 = 7 } ncclDataType_t;
typedef enum { ncclSum = 0, ncclProd = 1, ncclMax = 2, ncclMin = 3 } ncclRedOp_t;
}

namespace {

struct Rccl {
    void* handle = nullptr;
    ncclResult_t (*GetUniqueId)(ncclUniqueId*) = nullptr;
    ncclResult_t (*CommInitRank)(ncclComm_t*, int, ncclUniqueId, int) = nullptr;
    ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
    ncclResult_t (*CommAbort)(ncclComm_t) = nullptr;
    ncclResult_t (*GroupStart)() = nullptr;
    ncclResult_t (*GroupEnd)() = nullptr;
    ncclResult_t (*Send)(const void*, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*Recv)(void*, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*AllReduce)(const void*, void*, size_t, ncclDataType_t, ncclRedOp_t, ncclComm_t, hipStream_t) = nullptr;
    const char* (*GetErrorString)(ncclResult_t) = nullptr;
    bool ok() const { return handle != nullptr; }
} g_rccl;

using sobfu_hip::kHalo;
using sobfu_hip::kSlots;
using sobfu_hip::TileLay;
// iterations one solve may run on a handle whose max-norm rows other processes map (direct transport): the rows are part of the arena
// the peers open once, so their number is fixed at creation (16 MiB)
constexpr int kRowsIters = 16384;
constexpr int kSplitAMaxPlanes = 64;  // owned planes up to which pass A is split into boundary + interior launches
constexpr int kMaxSync = sobfu_hip::kMaxSync;
// The runtime carves allocations of up to GPU_MAX_SUBALLOC_SIZE (4 MiB by default) out of shared blocks, and hipIpcGetMemHandle
// refuses a pointer that is not the base of its block ("invalid argument", one start-up in ~10 on small test grids): whatever
// is exported to other processes is allocated at least this large, i.e. as a block of its own.
constexpr size_t kOwnBlock = (size_t) 8 << 20;

// Blocks that other processes map are never handed back to the runtime while the process lives: they are parked and reused by
// the next handle.  A block that has been exported keeps its 64-byte handle -- and the mappings the peers hold -- for good;
// exporting memory again after a free / re-allocation at the same address is what hipIpcGetMemHandle refused now and then
// when a process built several handles in a row (tile-grid autotuning).  One block per size class and kind in practice.
struct PooledBlock {
    void* ptr;
    size_t bytes;
    int device;
    bool uncached, in_use, has_handle;
    hipIpcMemHandle_t handle;
};
std::vector<PooledBlock> g_pool;
std::mutex g_pool_mutex;
// The export handle is taken when a block is allocated, and a block the runtime refuses to export is parked for good and
// replaced by another: hipIpcGetMemHandle now and then answers "invalid argument" for a perfectly ordinary fresh allocation
// (seen once in ~100 allocations when processes that had used IPC themselves had just exited) -- a second block has always worked.
int pool_take(void** out, size_t bytes, bool uncached) {
    std::lock_guard<std::mutex> lock(g_pool_mutex);
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return (int) hipGetLastError();
    PooledBlock* best = nullptr;  // best fit among the parked blocks of THIS device
    for (PooledBlock& b : g_pool)
        if (!b.in_use && b.device == dev && b.uncached == uncached && b.bytes >= bytes && (!best || b.bytes < best->bytes)) best = &b;
    if (best) {
        best->in_use = true;
        *out         = best->ptr;
        return 0;
    }
    for (int attempt = 0;; ++attempt) {
        void* p = nullptr;
        if (uncached && hipExtMallocWithFlags(&p, bytes, hipDeviceMallocUncached) != hipSuccess) {
            (void) hipGetLastError();
            p = nullptr;  // plain device memory if the runtime refuses (the flags are polled with system-scope loads either way)
        }
        if (!p) {
            hipError_t e = hipMalloc(&p, bytes);
            if (e != hipSuccess) return (int) e;
        }
        PooledBlock b{p, bytes, dev, uncached, true, false, {}};
        const hipError_t e = hipIpcGetMemHandle(&b.handle, p);
        b.has_handle = e == hipSuccess;
        if (!b.has_handle) (void) hipGetLastError();
        if (b.has_handle || attempt == 3) {  // (after four refusals the block is used as it is: only the direct transport needs the handle)
            g_pool.push_back(b);
            *out = p;
            return 0;
        }
        std::fprintf(stderr, "sobfu_hip: hipIpcGetMemHandle refused a fresh %zu-byte block (%s); parking it and taking another\n", bytes,
                     hipGetErrorString(e));
        b.uncached = !uncached;  // never matches a later request of this kind ...
        b.bytes    = 0;          // ... or of any size
        g_pool.push_back(b);
    }
}
void pool_give_back(void* p) {
    std::lock_guard<std::mutex> lock(g_pool_mutex);
    for (PooledBlock& b : g_pool)
        if (b.ptr == p) b.in_use = false;
}

#define RCCL_TRY(expr)                                                                          \
    do {                                                                                        \
        ncclResult_t _r = (expr);                                                               \
        if (_r != ncclSuccess) {                                                                \
            std::fprintf(stderr, "sobfu_hip: RCCL error %d (%s) at %s:%d\n", (int) _r,            \
                         g_rccl.GetErrorString ? g_rccl.GetErrorString(_r) : "?", __FILE__, __LINE__); \
            return SOBFU_E_RCCL;                                                                \
        }                                                                                       \
    } while (0)

using sobfu_hip::DevicePtr;
using sobfu_hip::EventPtr;
using sobfu_hip::StreamPtr;
struct PoolGiveBack {
    void operator()(void* p) const { pool_give_back(p); }
};
struct PlanDestroy {
    void operator()(sobfu_hip::TilePassAPlan* p) const { sobfu_hip::tile_pass_a_plan_destroy(p); }
};
struct CommDestroy {  // (abort_comms takes a communicator out with release() and aborts it instead)
    void operator()(ncclComm_t c) const {
        if (g_rccl.ok()) (void) g_rccl.CommDestroy(c);
    }
};
template <class T> using PooledPtr = std::unique_ptr<T, PoolGiveBack>;
using PlanPtr = std::unique_ptr<sobfu_hip::TilePassAPlan, PlanDestroy>;
using CommPtr = std::unique_ptr<ncclComm, CommDestroy>;

// The max-norm rows of a handle, kSlots words per iteration (row `it` belongs to iteration `it`, row 0 to none).  `slots`: the rows
// pass B folds this rank's maxima into.  The GLOBAL rows are the ones every rank stores its row maximum into (direct transport, and the
// handles that time its launches): kRowsIters + 2 of them sit in the arena the peers map, so a connected handle's capacity is fixed; an
// unconnected one may outgrow them into a private array.
struct MaxNormRows {
    DevicePtr<uint32_t> slots, own;  // own: the private global rows
    uint32_t* exported = nullptr;    // the global rows in the arena
    uint32_t* grows    = nullptr;    // the global rows in use: `exported` or `own`
    int iters          = 0;          // iterations a solve may run
    uint32_t* local(int it) const { return slots.get() + (size_t) it * kSlots; }
    // the rows the gate reads: global by the time it does
    const uint32_t* gate(bool sync) const { return sync ? grows : slots.get(); }
    // Room for a solve of `want` iterations.  fixed (connected, or about to connect): the exported rows, whatever the handle used
    // before.  The state is reset BEFORE anything is allocated (a failure leaves no rows and capacity 0), and the device's TileSync
    // learns where the global rows are whenever they move.
    int make_room(int want, bool fixed, sobfu_hip::TileSync* sync_d) {
        if (fixed && want > kRowsIters) return SOBFU_E_UNSUPPORTED;
        if (want <= iters && !(fixed && own)) return 0;
        const int n = fixed ? kRowsIters : std::max(want, kRowsIters);
        slots.reset();
        own.reset();
        grows = nullptr;
        iters = 0;
        SOBFU_HIP_TRY(sobfu_hip::device_alloc(slots, (size_t) (n + 1) * kSlots * 4));
        if (n > kRowsIters) {
            SOBFU_HIP_TRY(sobfu_hip::device_alloc(own, (size_t) (n + 2) * kSlots * 4));
            SOBFU_HIP_TRY(hipMemset(own.get(), 0, (size_t) (n + 2) * kSlots * 4));
        }
        uint32_t* g = own ? own.get() : exported;
        SOBFU_HIP_TRY(hipMemcpy(&sync_d->my_grows, &g, sizeof g, hipMemcpyHostToDevice));
        grows = g;
        iters = n;
        return 0;
    }
};

}  // namespace

// The members release what they hold, in the reverse order of their declaration.  THAT ORDER IS LOAD-BEARING: buffers, plans and
// events go first, then each stream followed by the communicator that used it.
struct sobfu_hip_tiled {
    int X, Y, Z, world, rank;
    TileLay lay;  // this rank's tile: owned cells, halo cells, local extents, the halo messages' cells (sobfu_tile_layout.hpp)
    sobfu_hip_solver_params p;
    float taps[7];
    CommPtr comm;
    StreamPtr comm_stream;
    // optional second communicator + stream for the max-norm all-reduce (sobfu_hip_tiled_add_reduce_comm): it then never queues
    // behind (or in front of) a halo exchange on the main communicator
    CommPtr comm2;
    StreamPtr red_stream;
    EventPtr ev_first, ev_row, ev_red[2], ev_xchg, ev_bnd;
    sobfu_hip_tiled_exchange_fn xfn = nullptr;    // transport of a communicator-less handle
    sobfu_hip_tiled_allreduce_fn rfn = nullptr;
    void* tctx = nullptr;
    size_t NL, NF;
    // the messages of one exchange: offsets into the packed buffers, the in-place z faces of a 3-D tile, n_packed
    sobfu_hip::TileMsgs mx;
    DevicePtr<uint32_t> scatter_table;  // destination cell of every cell of the packed receive buffer (the loop's scatter, precomputed)
    unsigned scatter_cells = 0;
    DevicePtr<float> recvbuf, sendbuf;
    // optional timing of an iteration's three pieces with HIP events on the loop's stream (sobfu_hip_tiled_set_profiling)
    int prof_stride = 0, prof_pending = 0, prof_n = 0;
    std::vector<EventPtr> prof_ev;
    double prof_ms[3] = {0, 0, 0};  // pass A, exchange (transfer + unpack; the direct transport has none), pass B
    // pass A's launch plans (box lists in device memory, see build_a_boxes), per nabla_U half: one push box per message + the owned
    // block, and the push boxes alone (sobfu_hip_tiled_probe_push); the whole owned block alone (launches without messages)
    PlanPtr a_own_plan, a_push_plan[2], a_plan[2];
    // direct transport (sobfu_hip_tiled_connect): push destinations in the peers, signalling state
    bool direct = false, dead = false, first_checked = false, dry_packed = false, force_comm = false;
    int debug_skip = 0;  // sobfu_hip::DebugSkip bits
    int wait_enabled = 1;
    DevicePtr<sobfu_hip::TileSync> sync_d;
    // what the peers map (direct transport): ONE arena [nabla_U half 0 | half 1 | global max-norm rows ((kRowsIters + 2) x 256)] and
    // the arrival flags [kMaxSync], uncached -- both padded to kOwnBlock so that hipIpcGetMemHandle accepts them
    PooledPtr<uint32_t> flags;
    MaxNormRows rows;
    PooledPtr<char> arena;
    size_t arena_bytes = 0, nu_off[2] = {0, 0}, rows_off = 0;
    // compact tile state (see sobfu_hip_solver_set_compact): 12-byte psi / nabla_U, tsdf-only F / G / phi_n.  psi and F = (phi_n o psi).tsdf
    // are ping-ponged (iteration k reads half (k-1)&1 and writes half k&1); nabla_U (two halves of the arena) is double-buffered by
    // iteration parity on the tile path (see the top of the file), the slab schedules use nUb[0].
    float* nUb[2] = {nullptr, nullptr};
    DevicePtr<float> c_n, c_g, c_f[2], c_psi[2];
    uint32_t seq_total = 0;                        // sequence numbers used so far (every rank counts the same)
    uint64_t timeout_ticks = 0;                    // deadline of the in-kernel waits (100 MHz ticks; SOBFU_TILED_DEADLINE_S at create)
    int schedule = 0;  // 0 heuristic, 1 overlapped + pass A split, 2 overlapped + pass A whole, 3 serial (sobfu_hip_tiled_set_schedule)
    double last_enqueue_us = 0.0;  // host time per iteration the last iterate() spent issuing the loop (diagnostics)
    struct Session {  // an open solve (tiled_begin .. tiled_end)
        bool active = false;
        const float* pn = nullptr;
        float *pnp = nullptr, *psi = nullptr;
        int cap = 0, launched = 0;
        bool flushed = false;  // the direct transport's end-of-solve handshake has been issued (test harnesses issue it as a phase)
        bool red_issued[2] = {false, false};
        int red_upto = 0;  // rows 1 .. red_upto have been (or are being) all-reduced
        uint32_t seq_base = 0;
    } q;
};

namespace {

double deadline_seconds() {
    const char* e = std::getenv("SOBFU_TILED_DEADLINE_S");
    const double v = e ? std::atof(e) : 0.0;
    return v > 0.0 ? v : 30.0;
}

// (re)builds pass A's box lists and their launch plans: one push box per message, then the owned block.  Destinations: the peers'
// halo cells when connected (dst[half][i] != null), else the packed send buffer.  On failure the handle keeps the plans it had.
int build_a_boxes(sobfu_hip_tiled* t, float* const* dst0, float* const* dst1, const TileLay* peers) {
    const sobfu_hip::PushBoxes pb = sobfu_hip::push_boxes(t->lay, t->mx, t->sendbuf.get(), dst0, dst1, peers, t->debug_skip);
    PlanPtr all[2], push[2], own_only;
    auto plan = [&](PlanPtr& out, const std::vector<sobfu_hip::TileLaunchBox>& v) {
        sobfu_hip::TilePassAPlan* p = nullptr;
        const int rc = sobfu_hip::tile_pass_a_plan_create(&p, v.data(), (int) v.size(), t->lay.a[0].L, t->lay.a[1].L, t->lay.a[2].L);
        out.reset(p);
        return rc;
    };
    for (int h = 0; h < 2; ++h) {
        std::vector<sobfu_hip::TileLaunchBox> v = pb.push[h];
        SOBFU_TRY(plan(push[h], v));
        sobfu_hip::TileLaunchBox own{};
        own.box = pb.own;
        v.push_back(own);
        SOBFU_TRY(plan(all[h], v));
    }
    // the same launch without messages (a world of one; timing experiments): the whole owned block
    sobfu_hip::TileLaunchBox whole{};
    whole.box = pb.whole;
    SOBFU_TRY(plan(own_only, {whole}));
    std::swap(all, t->a_plan);  // (the old plans go with the locals)
    std::swap(push, t->a_push_plan);
    std::swap(own_only, t->a_own_plan);
    return 0;
}

void abort_comms(sobfu_hip_tiled* t) {
    if (g_rccl.ok() && g_rccl.CommAbort) {
        if (t->comm2) (void) g_rccl.CommAbort(t->comm2.release());
        if (t->comm) (void) g_rccl.CommAbort(t->comm.release());
    }
    t->dead = true;
}

// Handles whose pass A signals and waits (and whose gate reads the global max-norm rows): the direct transport, and a bare dry handle
// (no communicator, no transport plugged in), which times the direct schedule -- or, with SOBFU_TILED_DRY_PACKED=1 at create, the
// launches of the RCCL / callback transports (pass A packing into the send buffer, the scatter kernel, pass B)
bool uses_sync(const sobfu_hip_tiled* t) { return t->direct || (!t->comm && !t->xfn && !t->dry_packed); }
bool tile_path(const sobfu_hip_tiled* t) { return !t->lay.slab() || uses_sync(t); }

// the image of the handle's TileSync without peers (sobfu_hip_tiled_connect adds them)
sobfu_hip::TileSync fill_sync(const sobfu_hip_tiled* t) {
    sobfu_hip::TileSync sy{};
    sy.my_rank = (uint32_t) t->rank; sy.world = (uint32_t) t->world;
    sy.timeout_ticks = t->timeout_ticks;
    sy.my_flags = t->flags.get(); sy.my_grows = t->rows.grows;
    return sy;
}

}  // namespace

extern "C" {

int sobfu_hip_tiled_load_rccl(const char* librccl_path) {
    if (g_rccl.ok()) return 0;
    SOBFU_CHECK_ARGS(librccl_path);
    void* h = dlopen(librccl_path, RTLD_NOW | RTLD_GLOBAL);
    if (!h) {
        std::fprintf(stderr, "sobfu_hip: cannot dlopen %s: %s\n", librccl_path, dlerror());
        return SOBFU_E_RCCL;
    }
#define SYM(field, name)                                         \
    *(void**) (&g_rccl.field) = dlsym(h, name);                  \
    if (!g_rccl.field) {                                         \
        std::fprintf(stderr, "sobfu_hip: %s has no %s\n", librccl_path, name); \
        return SOBFU_E_RCCL;                                     \
    }
    SYM(GetUniqueId, "ncclGetUniqueId")
    SYM(CommInitRank, "ncclCommInitRank")
    SYM(CommDestroy, "ncclCommDestroy")
    SYM(CommAbort, "ncclCommAbort")
    SYM(GroupStart, "ncclGroupStart")
    SYM(GroupEnd, "ncclGroupEnd")
    SYM(Send, "ncclSend")
    SYM(Recv, "ncclRecv")
    SYM(AllReduce, "ncclAllReduce")
    SYM(GetErrorString, "ncclGetErrorString")
#undef SYM
    g_rccl.handle = h;
    return 0;
}

int sobfu_hip_tiled_unique_id(char out[128]) {
    SOBFU_CHECK_ARGS(out);
    if (!g_rccl.ok()) return SOBFU_E_RCCL;
    ncclUniqueId id;
    RCCL_TRY(g_rccl.GetUniqueId(&id));
    static_assert(sizeof(id) == 128, "ncclUniqueId is 128 bytes");
    std::memcpy(out, &id, 128);
    return 0;
}

int sobfu_hip_tiled_destroy(sobfu_hip_tiled* t) {
    if (t) delete t;  // the members release what they hold (see the struct for the order)
    return 0;
}

int sobfu_hip_tiled_create3(sobfu_hip_tiled** out, int X, int Y, int Z, int Px, int Py, int Pz, int rank, const char unique_id[128],
                            const sobfu_hip_solver_params* params) {
    SOBFU_CHECK_ARGS(out && params && unique_id && X > 1 && Y > 1 && Z > 1 && Px >= 1 && Py >= 1 && Pz >= 1 && rank >= 0 &&
                     rank < Px * Py * Pz);
    bool dry = true;  // an all-zero id asks for a communicator-less handle: tile layout, kernels and stream choreography of
    for (int i = 0; i < 128; ++i) dry = dry && unique_id[i] == 0;  // (grid, rank); transport: sobfu_hip_tiled_set_transport / _connect
    if (!dry && !g_rccl.ok()) return SOBFU_E_RCCL;
    if (params->s < 7) return SOBFU_E_UNSUPPORTED;
    std::unique_ptr<sobfu_hip_tiled> t(new sobfu_hip_tiled());  // an early return releases whatever has been built
    t->X = X; t->Y = Y; t->Z = Z; t->world = Px * Py * Pz; t->rank = rank;
    const int dims[3] = {X, Y, Z}, P[3] = {Px, Py, Pz};
    t->lay = sobfu_hip::make_layout(dims, P, rank);
    if (!t->lay.ok) return SOBFU_E_UNSUPPORTED;
    // bring-up / timing settings of this handle, read once ("environment")
    const char* dp = std::getenv("SOBFU_TILED_DRY_PACKED");
    t->dry_packed = dp && dp[0] == '1';
    const char* fc = std::getenv("SOBFU_TILED_FORCE_COMM");
    t->force_comm = fc && fc[0] == '1';
    const char* ds = std::getenv("SOBFU_TILED_DEBUG_SKIP");
    t->debug_skip = ds ? std::atoi(ds) : 0;
    t->timeout_ticks = (uint64_t) (deadline_seconds() * 1e8);
    t->NL = t->lay.cells();
    t->NF = (size_t) X * Y * Z;
    t->p  = *params;
    float h[16];
    SOBFU_TRY(sobfu_hip_sobolev_filter(params->s, params->lambda, h));
    for (int i = 0; i < 7; ++i) t->taps[i] = h[i];
    t->mx = sobfu_hip::make_messages(t->lay);
    if (t->mx.floats > 0) {
        SOBFU_HIP_TRY(sobfu_hip::device_alloc(t->sendbuf, t->mx.floats * sizeof(float)));
        SOBFU_HIP_TRY(sobfu_hip::device_alloc(t->recvbuf, t->mx.floats * sizeof(float)));
    }
    if (!t->lay.slab() && t->mx.n_packed > 0) {  // where every cell of the packed receive buffer goes
        const std::vector<uint32_t> tab = sobfu_hip::scatter_table(t->lay, t->mx.n_packed);
        t->scatter_cells = (unsigned) tab.size();
        SOBFU_HIP_TRY(sobfu_hip::device_alloc(t->scatter_table, tab.size() * sizeof(uint32_t)));
        SOBFU_HIP_TRY(hipMemcpy(t->scatter_table.get(), tab.data(), tab.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    }
    auto up = [](size_t v) { return (v + 4095) & ~(size_t) 4095; };
    t->nu_off[0] = 0;
    t->nu_off[1] = up(t->NL * 12);
    t->rows_off  = t->nu_off[1] + up(t->NL * 12);
    t->arena_bytes = std::max(t->rows_off + up((size_t) (kRowsIters + 2) * kSlots * 4), kOwnBlock);
    void* block = nullptr;
    SOBFU_TRY(pool_take(&block, t->arena_bytes, false));
    t->arena.reset((char*) block);
    t->nUb[0] = (float*) (t->arena.get() + t->nu_off[0]);
    t->nUb[1] = (float*) (t->arena.get() + t->nu_off[1]);
    t->rows.exported = (uint32_t*) (t->arena.get() + t->rows_off);
    // halo cells no message fills (tile corners) stay finite; rows start at "converged nowhere" = 0 (blocking: the loop's
    // streams do not order against the null stream)
    SOBFU_HIP_TRY(hipMemset(t->arena.get(), 0, t->arena_bytes));
    for (int k = 0; k < 2; ++k) {
        SOBFU_HIP_TRY(sobfu_hip::device_alloc(t->c_psi[k], t->NL * 12));
        SOBFU_HIP_TRY(sobfu_hip::device_alloc(t->c_f[k], t->NL * 4));
    }
    SOBFU_HIP_TRY(sobfu_hip::device_alloc(t->c_g, t->NL * 4));
    SOBFU_HIP_TRY(sobfu_hip::device_alloc(t->c_n, t->NF * 4));
    // arrival flags: written by the peers over xGMI, polled here -- uncached memory, so that neither side's L2 sits between
    // a store and the poll (plain device memory if the runtime refuses)
    SOBFU_TRY(pool_take(&block, kOwnBlock, true));
    t->flags.reset((uint32_t*) block);
    SOBFU_HIP_TRY(hipMemset(t->flags.get(), 0, kMaxSync * sizeof(uint32_t)));
    SOBFU_HIP_TRY(sobfu_hip::device_alloc(t->sync_d, sizeof(sobfu_hip::TileSync)));
    // max-norm rows for kRowsIters iterations up front: a solve never reallocates inside a timed region
    SOBFU_TRY(t->rows.make_room(kRowsIters, false, t->sync_d.get()));
    const sobfu_hip::TileSync sy = fill_sync(t.get());
    SOBFU_HIP_TRY(hipMemcpy(t->sync_d.get(), &sy, sizeof sy, hipMemcpyHostToDevice));
    SOBFU_TRY(build_a_boxes(t.get(), nullptr, nullptr, nullptr));
    hipStream_t cs = nullptr;
    SOBFU_HIP_TRY(hipStreamCreateWithFlags(&cs, hipStreamNonBlocking));
    t->comm_stream.reset(cs);
    // the max-norm rows are written by pass B's atomics on this device, but a real RCCL all-reduce may let PEERS write the
    // reduced row straight into this buffer (direct / registered-buffer paths): every event keeps the system-scope fence
    // (a fence-less variant -- an L2 write-back + invalidate less per edge -- would have to be validated on >= 2 real GPUs first).
    for (EventPtr* e : {&t->ev_bnd, &t->ev_xchg, &t->ev_first, &t->ev_red[0], &t->ev_red[1], &t->ev_row})
        SOBFU_HIP_TRY(sobfu_hip::event_create(*e, hipEventDisableTiming));
    if (!dry) {
        ncclUniqueId id;
        std::memcpy(&id, unique_id, 128);
        ncclComm_t c     = nullptr;
        ncclResult_t r = g_rccl.CommInitRank(&c, t->world, id, rank);
        if (r != ncclSuccess) {
            std::fprintf(stderr, "sobfu_hip: ncclCommInitRank failed: %s\n", g_rccl.GetErrorString(r));
            return SOBFU_E_RCCL;
        }
        t->comm.reset(c);
    }
    // hipMemset / hipMemcpy on device memory may return before they have run.  The arrays cleared above are about to be mapped and
    // written by OTHER processes, which no stream of this one orders against: a clear that ran late would wipe a peer's first
    // arrival flag (seen: one hang in ~10 start-ups with four ranks sharing a GPU) -- drain the device before anybody can see them.
    SOBFU_HIP_TRY(hipDeviceSynchronize());
    *out = t.release();
    return 0;
}

int sobfu_hip_tiled_create(sobfu_hip_tiled** out, int X, int Y, int Z, int world, int rank, const char unique_id[128],
                           const sobfu_hip_solver_params* params) {
    return sobfu_hip_tiled_create3(out, X, Y, Z, 1, 1, world, rank, unique_id, params);  // z-slabs
}

// ---- direct transport -------------------------------------------------------------------------------------------------------
int sobfu_hip_ipc_export(const void* d_ptr, char handle[64]) {
    SOBFU_CHECK_ARGS(d_ptr && handle);
    static_assert(sizeof(hipIpcMemHandle_t) == 64, "hipIpcMemHandle_t is 64 bytes");
    {
        std::lock_guard<std::mutex> lock(g_pool_mutex);
        for (const PooledBlock& b : g_pool)  // the library's own blocks were exported when they were allocated
            if (b.ptr == d_ptr && b.has_handle) {
                std::memcpy(handle, &b.handle, 64);
                return 0;
            }
    }
    hipIpcMemHandle_t h;
    SOBFU_HIP_TRY(hipIpcGetMemHandle(&h, const_cast<void*>(d_ptr)));
    std::memcpy(handle, &h, 64);
    return 0;
}
int sobfu_hip_ipc_open(const char handle[64], void** d_ptr) {
    SOBFU_CHECK_ARGS(handle && d_ptr);
    hipIpcMemHandle_t h;
    std::memcpy(&h, handle, 64);
    SOBFU_HIP_TRY(hipIpcOpenMemHandle(d_ptr, h, hipIpcMemLazyEnablePeerAccess));
    return 0;
}
int sobfu_hip_ipc_close(void* d_ptr) {
    if (!d_ptr) return 0;
    SOBFU_HIP_TRY(hipIpcCloseMemHandle(d_ptr));
    return 0;
}

int sobfu_hip_tiled_exports_get(const sobfu_hip_tiled* t, sobfu_hip_tiled_exports* out) {
    SOBFU_CHECK_ARGS(t && out);
    out->arena = t->arena.get(); out->nabla_u_off[0] = t->nu_off[0]; out->nabla_u_off[1] = t->nu_off[1]; out->rows_off = t->rows_off;
    out->flags = t->flags.get();
    return 0;
}

int sobfu_hip_tiled_connect(sobfu_hip_tiled* t, int n_peers, const int* peer_ranks, const sobfu_hip_tiled_exports* peers) {
    SOBFU_CHECK_ARGS(t && n_peers >= 0 && (n_peers == 0 || (peer_ranks && peers)) && !t->q.active && !t->comm);
    if (t->world > kMaxSync) return SOBFU_E_UNSUPPORTED;
    // Cells other GPUs stored are read at system scope, which only the pipelined march of pass B does (sobfu_hip::pass_b_march): it
    // needs 32-bit gather offsets (phi_n below 2^30 voxels) and buffer addressing (the local arrays below 4 GiB).  Refused HERE, not by
    // a launch in the middle of a solve whose pass A has already pushed into the peers.
    sobfu_hip::PassBMarch m;
    const sobfu_hip::PassBAsk connected{true, false, true, true};
    if (sobfu_hip::pass_b_march(sobfu_hip::grid_traits(t->lay.a[0].L, t->lay.a[1].L, t->lay.a[2].L, t->X, t->Y, t->Z, 0), connected, &m) != 0) return SOBFU_E_UNSUPPORTED;
    // (a longer solve on the unconnected handle may have moved the rows to a private array: back to the exported ones)
    SOBFU_TRY(t->rows.make_room(kRowsIters, true, t->sync_d.get()));
    const int dims[3] = {t->X, t->Y, t->Z};
    auto find = [&](int r) -> const sobfu_hip_tiled_exports* {
        for (int i = 0; i < n_peers; ++i)
            if (peer_ranks[i] == r) return &peers[i];
        return nullptr;
    };
    // push destinations: every message needs its peer
    std::vector<float*> d0(t->lay.msgs.size()), d1(t->lay.msgs.size());
    std::vector<TileLay> pl;
    for (size_t i = 0; i < t->lay.msgs.size(); ++i) {
        const sobfu_hip_tiled_exports* e = find(t->lay.msgs[i].peer);
        if (!e || !e->arena || !e->flags) return SOBFU_E_BADARG;
        d0[i] = (float*) ((char*) e->arena + e->nabla_u_off[0]);
        d1[i] = (float*) ((char*) e->arena + e->nabla_u_off[1]);
        pl.push_back(sobfu_hip::make_layout(dims, t->lay.P, t->lay.msgs[i].peer));
    }
    // sync set: EVERY other rank -- the halo neighbours for the nabla_U cells, the rest because the max-norm rows become global by
    // every rank storing its row maximum at every other rank (world <= 64: a few 4-byte stores per iteration)
    sobfu_hip::TileSync sy = fill_sync(t);
    for (int r = 0; r < t->world; ++r) {
        if (r == t->rank) continue;
        const sobfu_hip_tiled_exports* e = find(r);
        if (!e || !e->flags || !e->arena) return SOBFU_E_BADARG;
        sy.sync_rank[sy.n_sync]  = r;
        sy.peer_flags[sy.n_sync] = (uint32_t*) e->flags;
        sy.peer_grows[sy.n_sync] = (uint32_t*) ((char*) e->arena + e->rows_off);
        sy.n_sync += 1;
    }
    SOBFU_HIP_TRY(hipMemcpy(t->sync_d.get(), &sy, sizeof sy, hipMemcpyHostToDevice));
    SOBFU_HIP_TRY(hipDeviceSynchronize());
    SOBFU_TRY(build_a_boxes(t, d0.data(), d1.data(), pl.data()));
    t->direct = true;
    return 0;
}

int sobfu_hip_tiled_max_iterations(const sobfu_hip_tiled* t) { return t ? (t->direct ? kRowsIters : 0x7fffffff) : 0; }

int sobfu_hip_p2p_info(int device, int peer_device, int out[4]) {
    SOBFU_CHECK_ARGS(out && device >= 0 && peer_device >= 0);
    int can = 0, rank = -1;
    uint32_t link = 0, hops = 0;
    out[0] = out[1] = out[2] = out[3] = -1;
    if (device == peer_device) {
        out[0] = 1; out[1] = 0; out[2] = 0; out[3] = 0;
        return 0;
    }
    if (hipDeviceCanAccessPeer(&can, device, peer_device) != hipSuccess) (void) hipGetLastError(); else out[0] = can;
    if (hipExtGetLinkTypeAndHopCount(device, peer_device, &link, &hops) != hipSuccess) (void) hipGetLastError();
    else { out[1] = (int) link; out[2] = (int) hops; }
    if (hipDeviceGetP2PAttribute(&rank, hipDevP2PAttrPerformanceRank, device, peer_device) != hipSuccess) (void) hipGetLastError(); else out[3] = rank;
    return 0;
}

int sobfu_hip_tiled_wait_stats(sobfu_hip_tiled* t, double* wait_us, int* waits, int reset) {
    SOBFU_CHECK_ARGS(t);
    sobfu_hip::TileSync sy;
    SOBFU_HIP_TRY(hipMemcpy(&sy, t->sync_d.get(), sizeof sy, hipMemcpyDeviceToHost));
    if (wait_us) *wait_us = (double) sy.wait_ticks / 100.0;  // wall_clock64: 100 MHz
    if (waits) *waits = (int) sy.wait_count;
    if (reset) {
        const uint64_t z[2] = {0, 0};
        SOBFU_HIP_TRY(hipMemcpy(&t->sync_d->wait_ticks, z, 16, hipMemcpyHostToDevice));
    }
    return 0;
}

// diagnostics of a CONNECTED handle outside a solve; every rank of the world makes the same calls in the same order (the sequence
// numbers of the arrival flags advance in step)
int sobfu_hip_tiled_pingpong(sobfu_hip_tiled* t, int rank_a, int rank_b, int reps, void* stream) {
    SOBFU_CHECK_ARGS(t && t->direct && !t->q.active && reps > 0 && rank_a != rank_b && rank_a >= 0 && rank_b >= 0 && rank_a < t->world && rank_b < t->world);
    if (t->dead) return SOBFU_E_TIMEOUT;
    const uint32_t seq0 = t->seq_total + 1u;
    t->seq_total += 2u * (uint32_t) reps;
    if (t->rank != rank_a && t->rank != rank_b) return 0;
    const int other = t->rank == rank_a ? rank_b : rank_a;
    const int q     = other < t->rank ? other : other - 1;  // the sync set lists every other rank in rank order
    return sobfu_hip::launch_tile_pingpong(t->sync_d.get(), q, t->rank == rank_a ? 1 : 0, seq0, reps, (hipStream_t) stream);
}

int sobfu_hip_tiled_probe_push(sobfu_hip_tiled* t, int reps, void* stream) {
    SOBFU_CHECK_ARGS(t && uses_sync(t) && !t->q.active && reps > 0);  // handles whose pass A signals
    if (t->dead) return SOBFU_E_TIMEOUT;
    for (int r = 0; r < reps; ++r) {
        const uint32_t seq = ++t->seq_total;
        // pass A's push boxes alone, on whatever the compact state holds (the halo rims they fill are scratch between solves); no
        // messages: no launch
        SOBFU_TRY(sobfu_hip::launch_tile_pass_a_plan(t->a_push_plan[seq & 1u].get(), t->c_f[0].get(), t->c_g.get(), t->c_psi[0].get(), t->nUb[seq & 1u],
                                                     t->p.w_reg, t->sync_d.get(), seq, t->wait_enabled, nullptr, 0, (hipStream_t) stream));
    }
    return 0;
}

int sobfu_hip_tiled_set_wait(sobfu_hip_tiled* t, int wait) {
    SOBFU_CHECK_ARGS(t);
    t->wait_enabled = wait ? 1 : 0;
    return 0;
}

int sobfu_hip_tiled_status(sobfu_hip_tiled* t, int* missing_peer) {
    SOBFU_CHECK_ARGS(t);
    uint32_t err = 0;
    SOBFU_HIP_TRY(hipMemcpy(&err, &t->sync_d->err, 4, hipMemcpyDeviceToHost));
    if (missing_peer) *missing_peer = err ? (int) err - 1 : -1;
    return (err || t->dead) ? SOBFU_E_TIMEOUT : 0;
}

int sobfu_hip_tiled_set_transport(sobfu_hip_tiled* t, sobfu_hip_tiled_exchange_fn exchange_fn, sobfu_hip_tiled_allreduce_fn allreduce_fn,
                                  void* ctx) {
    SOBFU_CHECK_ARGS(t && !t->comm);
    t->xfn = exchange_fn;
    t->rfn = allreduce_fn;
    t->tctx = ctx;
    return 0;
}

int sobfu_hip_tiled_add_reduce_comm(sobfu_hip_tiled* t, const char unique_id[128]) {
    SOBFU_CHECK_ARGS(t && unique_id && t->comm && !t->comm2);
    ncclUniqueId id;
    std::memcpy(&id, unique_id, 128);
    ncclComm_t c = nullptr;
    RCCL_TRY(g_rccl.CommInitRank(&c, t->world, id, t->rank));
    t->comm2.reset(c);
    hipStream_t rs = nullptr;
    SOBFU_HIP_TRY(hipStreamCreateWithFlags(&rs, hipStreamNonBlocking));
    t->red_stream.reset(rs);
    return 0;
}

int sobfu_hip_tiled_set_schedule(sobfu_hip_tiled* t, int schedule) {
    SOBFU_CHECK_ARGS(t && schedule >= 0 && schedule <= 3);
    t->schedule = schedule;
    return 0;
}

double sobfu_hip_tiled_last_enqueue_us(const sobfu_hip_tiled* t) { return t ? t->last_enqueue_us : 0.0; }

int sobfu_hip_tiled_set_profiling(sobfu_hip_tiled* t, int stride, int max_samples) {
    SOBFU_CHECK_ARGS(t && stride >= 0 && max_samples >= 0);
    t->prof_stride = stride;
    while (stride > 0 && t->prof_ev.size() < (size_t) 4 * max_samples) {  // created here, never inside a timed region
        EventPtr e;
        SOBFU_HIP_TRY(sobfu_hip::event_create(e, hipEventDefault));
        t->prof_ev.push_back(std::move(e));
    }
    return 0;
}

int sobfu_hip_tiled_get_profile(sobfu_hip_tiled* t, float ms[3], int* samples, int reset) {
    SOBFU_CHECK_ARGS(t && ms);
    for (int k = 0; k < t->prof_pending; ++k) {  // the caller has synchronised the stream
        for (int j = 0; j < 3; ++j) {
            float v = 0;
            SOBFU_HIP_TRY(hipEventElapsedTime(&v, t->prof_ev[4 * k + j].get(), t->prof_ev[4 * k + j + 1].get()));
            t->prof_ms[j] += v;
        }
        t->prof_n += 1;
    }
    t->prof_pending = 0;
    for (int j = 0; j < 3; ++j) ms[j] = (float) t->prof_ms[j];
    if (samples) *samples = t->prof_n;
    if (reset) {
        t->prof_ms[0] = t->prof_ms[1] = t->prof_ms[2] = 0;
        t->prof_n = 0;
    }
    return 0;
}

int sobfu_hip_tiled_layout(const sobfu_hip_tiled* t, int* z0, int* z1, int* lo, int* hi, int* Lz, int* zbase) {
    SOBFU_CHECK_ARGS(t);
    const sobfu_hip::AxisLay& z = t->lay.a[2];
    if (z0) *z0 = z.g0;
    if (z1) *z1 = z.g1;
    if (lo) *lo = z.lo;
    if (hi) *hi = z.hi;
    if (Lz) *Lz = z.L;
    if (zbase) *zbase = z.base;
    return 0;
}

int sobfu_hip_tiled_layout3(const sobfu_hip_tiled* t, int out[24]) {
    SOBFU_CHECK_ARGS(t && out);
    for (int a = 0; a < 3; ++a) {
        const sobfu_hip::AxisLay& l = t->lay.a[a];
        out[a] = t->lay.P[a]; out[3 + a] = t->lay.c[a]; out[6 + a] = l.g0; out[9 + a] = l.g1; out[12 + a] = l.lo;
        out[15 + a] = l.hi; out[18 + a] = l.L; out[21 + a] = l.base;
    }
    return 0;
}

int sobfu_hip_tiled_messages(const sobfu_hip_tiled* t, sobfu_hip_tiled_msg* msgs, int* send_boxes, int* recv_boxes, int max_msgs) {
    if (!t) return SOBFU_E_BADARG;
    const int n = (int) t->mx.msgs.size();
    for (int i = 0; i < n && i < max_msgs; ++i) {
        if (msgs) msgs[i] = t->mx.msgs[i];
        if (send_boxes) std::memcpy(send_boxes + 6 * i, t->lay.msgs[i].sb, 6 * sizeof(int));
        if (recv_boxes) std::memcpy(recv_boxes + 6 * i, t->lay.msgs[i].rb, 6 * sizeof(int));
    }
    return n;  // number of messages of an exchange
}

int sobfu_hip_tiled_messages_inplace(const sobfu_hip_tiled* t, sobfu_hip_tiled_msg* msgs, int max_msgs, int* n_packed) {
    if (!t) return SOBFU_E_BADARG;
    if (n_packed) *n_packed = t->mx.n_packed;
    const int n = (int) t->mx.zmsgs.size();
    for (int i = 0; i < n && i < max_msgs; ++i)
        if (msgs) msgs[i] = t->mx.zmsgs[i];
    return n;
}

// Delivers the messages of one exchange from d_send to d_recv (RCCL grouped send/recv, or the user transport) and, in the same RCCL
// group, a second list with its own base pointers (the in-place z faces of a 3-D tile: both bases are the field array itself).
static int transfer(sobfu_hip_tiled* t, const float* d_send, float* d_recv, const sobfu_hip_tiled_msg* msgs, int n, hipStream_t stream,
                    const float* d_send2 = nullptr, float* d_recv2 = nullptr, const sobfu_hip_tiled_msg* msgs2 = nullptr, int n2 = 0) {
    if (n + n2 == 0) return 0;
    const struct { const float* send; float* recv; const sobfu_hip_tiled_msg* msgs; int n; } lists[2] = {{d_send, d_recv, msgs, n}, {d_send2, d_recv2, msgs2, n2}};
    if (!t->comm) {  // user transport / dry handle: one call per list (a transport sees at most one message per peer in a call)
        for (const auto& l : lists)
            if (t->xfn && l.n > 0) SOBFU_TRY(t->xfn(t->tctx, t->rank, l.send, l.recv, l.msgs, l.n, (void*) stream));
        return 0;
    }
    RCCL_TRY(g_rccl.GroupStart());
    for (const auto& l : lists)
        for (int i = 0; i < l.n; ++i) {
            RCCL_TRY(g_rccl.Send(l.send + l.msgs[i].send_off, l.msgs[i].count, ncclFloat32, l.msgs[i].peer, t->comm.get(), stream));
            RCCL_TRY(g_rccl.Recv(l.recv + l.msgs[i].recv_off, l.msgs[i].count, ncclFloat32, l.msgs[i].peer, t->comm.get(), stream));
        }
    RCCL_TRY(g_rccl.GroupEnd());
    return 0;
}

// z-slab schedules: `planes` owned planes per interior face of a slab field travel in place (no copy on either side)
static int exchange_planes(sobfu_hip_tiled* t, float* field3, int planes, hipStream_t stream) {
    const size_t plane_f = (size_t) t->X * t->Y * 3, cnt = plane_f * planes;
    sobfu_hip_tiled_msg m[2];
    int n = 0;
    if (t->rank > 0) m[n++] = {t->rank - 1, plane_f * t->lay.a[2].o0, plane_f * (t->lay.a[2].o0 - planes), cnt};
    if (t->rank < t->world - 1) m[n++] = {t->rank + 1, plane_f * (t->lay.a[2].o1 - planes), plane_f * t->lay.a[2].o1, cnt};
    return transfer(t, field3, field3, m, n, stream);
}

// tile path, RCCL / callback transports: the send buffer (filled by pass A's push boxes) -> peers -> scatter into the halo cells
// The z FACES do not go through the buffers: the neighbour across a z face has the same x / y layout, so 4 whole padded planes of the
// array (Lx x Ly x 4 cells: + 6 % bytes on a 132^2 plane) leave straight out of the owned rim and land straight in the halo planes --
// no push box packs them, the scatter kernel does not touch them.  What arrives in those planes' x / y halo columns is the sender's own
// (stale) halo content: exactly the cells of the xz / yz EDGE STRIPS, which the scatter -- behind the transfer on the same stream --
// overwrites with the diagonal neighbours' cells; the corner regions beyond are never read (every stencil is axis-aligned).
static int exchange_packed(sobfu_hip_tiled* t, float* field3, hipStream_t stream) {
    const int n = t->mx.n_packed, nz = (int) t->mx.zmsgs.size();
    if (n + nz == 0) return 0;
    SOBFU_TRY(transfer(t, t->sendbuf.get(), t->recvbuf.get(), t->mx.msgs.data(), n, stream, field3, field3, t->mx.zmsgs.data(), nz));
    if (t->scatter_table) return sobfu_hip::launch_msg_scatter_table(field3, t->recvbuf.get(), t->scatter_table.get(), t->scatter_cells, stream);
    return sobfu_hip::launch_msg_copy(false, field3, t->recvbuf.get(), t->lay.a[0].L, t->lay.a[1].L, t->lay.a[2].L, sobfu_hip::flat_boxes(t->lay, n, true).data(), n, stream);
}

static int allreduce_max(sobfu_hip_tiled* t, uint32_t* buf, size_t n, hipStream_t stream, bool own_comm = false) {
    if (!t->comm) return t->rfn ? t->rfn(t->tctx, t->rank, buf, n, (void*) stream) : 0;
    RCCL_TRY(g_rccl.AllReduce(buf, buf, n, ncclUint32, ncclMax, (own_comm ? t->comm2 : t->comm).get(), stream));
    return 0;
}

// Debug / bring-up: one halo exchange of a caller-provided 12-byte tile field exactly as the loop's RCCL / callback transports do
// it (z-slabs: `planes` planes in place; 3-D tiles: pack, transfer, scatter).
int sobfu_hip_tiled_exchange(sobfu_hip_tiled* t, float* d_field3, int planes, void* stream) {
    SOBFU_CHECK_ARGS(t && d_field3 && planes > 0 && planes <= kHalo && (t->lay.slab() || planes == kHalo));
    if (t->lay.slab()) return exchange_planes(t, d_field3, planes, (hipStream_t) stream);
    const int n = t->mx.n_packed;  // (the z faces travel in place: nothing to pack)
    if (n + (int) t->mx.zmsgs.size() == 0) return 0;
    SOBFU_TRY(sobfu_hip::launch_msg_copy(true, d_field3, t->sendbuf.get(), t->lay.a[0].L, t->lay.a[1].L, t->lay.a[2].L, sobfu_hip::flat_boxes(t->lay, n, false).data(), n, (hipStream_t) stream));
    return exchange_packed(t, d_field3, (hipStream_t) stream);
}

// Bring-up self test usable with ONE rank: a world-1 communicator sends n floats from d_src to itself into d_dst through
// the same group{send, recv} path the loop uses (RCCL allows self send/recv inside a group).
int sobfu_hip_tiled_self_sendrecv(sobfu_hip_tiled* t, const float* d_src, float* d_dst, size_t n, void* stream) {
    SOBFU_CHECK_ARGS(t && t->comm && d_src && d_dst && n > 0);
    RCCL_TRY(g_rccl.GroupStart());
    RCCL_TRY(g_rccl.Send(d_src, n, ncclFloat32, t->rank, t->comm.get(), (hipStream_t) stream));
    RCCL_TRY(g_rccl.Recv(d_dst, n, ncclFloat32, t->rank, t->comm.get(), (hipStream_t) stream));
    RCCL_TRY(g_rccl.GroupEnd());
    return 0;
}

int sobfu_hip_tiled_allreduce_max_u32(sobfu_hip_tiled* t, uint32_t* d_buf, size_t n, void* stream) {
    SOBFU_CHECK_ARGS(t && t->comm && d_buf && n > 0);
    RCCL_TRY(g_rccl.AllReduce(d_buf, d_buf, n, ncclUint32, ncclMax, t->comm.get(), (hipStream_t) stream));
    return 0;
}

// The gradient-descent loop (reference src/sobfu/cuda/solver.cu:106-193) on this rank's tile, in three pieces (begin / step / end;
// sobfu_hip_tiled_iterate = all three).  API-format arguments: d_phi_global_local / d_phi_n_psi_local float2 (Lx, Ly, Lz),
// d_phi_n_full float2 (X, Y, Z), d_psi_local float4 (Lx, Ly, Lz) whose owned cells and one-cell shells are exact on entry
// (identity: sobfu_hip_tile3_init_identity) and on exit.
//
// Convergence without a stall: psi and F = (phi_n o psi).tsdf are PING-PONGED (iteration k reads buffer (k-1)&1 and writes
// buffer k&1), and the device-side gate of iteration k looks at the max-norm row of iteration k-2.  When the threshold fires
// at iteration k, iteration k+1 has already run speculatively -- into the OTHER buffer -- every later launch is a no-op,
// and the state the reference's `break` (solver.cu:183) leaves is intact in buffer k&1.  The reduction that makes row k
// global therefore has a whole iteration to complete: on the direct transport it rides on pass A of iteration k+1 (every rank
// stores its row maximum at every other rank, covered by that iteration's arrival flags); on the others it is an all-reduce
// behind the exchange.  Nothing in the loop ever waits for a reduction that is still in flight (a same-iteration gate costs an
// exposed collective or a stream round trip per iteration: 67 vs 55 us per iteration in the round-2 N = 8 compute-side timing).

static int tiled_begin(sobfu_hip_tiled* t, const float* d_phi_global_local, const float* d_phi_n_full, float* d_phi_n_psi_local,
                       float* d_psi_local, int max_iters, hipStream_t st) {
    sobfu_hip_tiled::Session& q = t->q;
    if (q.active) return SOBFU_E_BADARG;
    if (t->dead) return SOBFU_E_TIMEOUT;
    const int X = t->X, Y = t->Y, Z = t->Z, Lx = t->lay.a[0].L, Ly = t->lay.a[1].L, Lz = t->lay.a[2].L;
    // the global rows of a connected handle are mapped by the peers: their number is fixed (sobfu_hip_tiled_max_iterations)
    const int rc = t->rows.make_room(max_iters, t->direct, t->sync_d.get());
    if (rc == SOBFU_E_UNSUPPORTED)
        std::fprintf(stderr, "sobfu_hip: a solve of %d iterations exceeds the %d the direct transport's peer-mapped max-norm rows hold; "
                             "split the solve or use the RCCL transport\n", max_iters, kRowsIters);
    SOBFU_TRY(rc);
    sobfu_hip_tiled::Session n{};
    n.pn = d_phi_n_full; n.pnp = d_phi_n_psi_local; n.psi = d_psi_local;
    n.cap = max_iters;
    n.seq_base = t->seq_total;
    // enter the compact format (includes the warp of solver.cu:106); both halves start equal so that cells no launch
    // writes (beyond the one-cell shells) hold the caller's values whichever half the loop ends in
    float *psi0 = t->c_psi[0].get(), *f0 = t->c_f[0].get();
    SOBFU_TRY(sobfu_hip::launch_pack_vec(d_psi_local, psi0, t->NL, st));
    SOBFU_TRY(sobfu_hip::launch_extract_tsdf(d_phi_global_local, t->c_g.get(), t->NL, st));
    SOBFU_TRY(sobfu_hip::launch_extract_tsdf(d_phi_n_full, t->c_n.get(), t->NF, st));
    SOBFU_TRY(sobfu_hip::launch_apply_tsdf_only(t->c_n.get(), f0, psi0, Lx, Ly, Lz, st, Z, X, Y));
    SOBFU_HIP_TRY(hipMemcpyAsync(t->c_psi[1].get(), psi0, t->NL * 12, hipMemcpyDeviceToDevice, st));
    SOBFU_HIP_TRY(hipMemcpyAsync(t->c_f[1].get(), f0, t->NL * 4, hipMemcpyDeviceToDevice, st));
    if (max_iters > 0) SOBFU_HIP_TRY(hipMemsetAsync(t->rows.local(0), 0, (size_t) (max_iters + 1) * kSlots * 4, st));
    q        = n;  // the session is open only once everything above has been enqueued
    q.active = true;
    return 0;
}

// the first iteration of a communicator's life, under a host-side deadline: a wedged rank says what it is waiting for and
// aborts its communicators instead of sitting in a collective until somebody's process-group timeout
static int first_iteration_watchdog(sobfu_hip_tiled* t, hipStream_t st) {
    t->first_checked = true;
    SOBFU_HIP_TRY(hipEventRecord(t->ev_first.get(), st));
    const double limit = deadline_seconds();
    const auto t0 = std::chrono::steady_clock::now();
    for (;;) {
        const hipError_t e = hipEventQuery(t->ev_first.get());
        if (e == hipSuccess) return 0;
        if (e != hipErrorNotReady) return (int) e;
        if (std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() > limit) break;
        std::this_thread::sleep_for(std::chrono::microseconds(200));
    }
    std::fprintf(stderr, "sobfu_hip: rank %d: the first tiled iteration has not completed after %.0f s -- waiting for the halo exchange "
                         "(grouped ncclSend/ncclRecv with ranks", t->rank, limit);
    for (const sobfu_hip_tiled_msg& m : t->mx.msgs) std::fprintf(stderr, " %d", m.peer);
    std::fprintf(stderr, ")%s; aborting the communicator(s)\n", t->p.max_update_norm >= 0.f ? " or the max-norm all-reduce" : "");
    abort_comms(t);
    return SOBFU_E_TIMEOUT;
}

// Where the all-reduce of a max-norm row runs on the RCCL / callback transports (the late gate gives row j until pass B of
// iteration j+2): in line behind pass B (serial / tile path), on the comm stream behind the next exchange (overlapped slab
// schedules), or -- opt-in, sobfu_hip_tiled_add_reduce_comm -- on a communicator and stream of its own.
enum Reduce { RED_NONE, RED_INLINE, RED_COMM_STREAM, RED_OWN_COMM };

// What one call into the loop needs to know about its handle, worked out once (tiled_end reads the same flags).
struct LoopCtx {
    sobfu_hip_tiled* t;
    hipStream_t st;
    int phases;  // 1 = pass A (+ the exchange of the RCCL / callback transports), 2 = pass B (+ the row reduction); 3 = a whole iteration
    bool can_converge;
    bool multi;   // the communication choreography runs
    bool tiles;   // the tile path (else a z-slab schedule) ...
    bool sync;    // ... whose pass A signals and waits (uses_sync)
    bool serial, split_a;  // z-slab schedules
    Reduce red_mode;
    sobfu_hip::PlaneRanges z;
    int own[6];  // the owned box
};
static LoopCtx loop_context(sobfu_hip_tiled* t, hipStream_t st, int phases) {
    LoopCtx c{};
    c.t = t; c.st = st; c.phases = phases;
    const sobfu_hip::AxisLay &lx = t->lay.a[0], &ly = t->lay.a[1], &lz = t->lay.a[2];
    const int own[6] = {lx.o0, lx.o1, ly.o0, ly.o1, lz.o0, lz.o1};
    for (int i = 0; i < 6; ++i) c.own[i] = own[i];
    c.z = sobfu_hip::plane_ranges(t->lay);
    // (SOBFU_TILED_FORCE_COMM=1 at create runs the communication choreography -- streams, events, empty exchange group, world-1
    // all-reduce -- on a single rank too: bring-up / test hook for 1-GPU machines)
    c.can_converge = t->p.max_update_norm >= 0.f;
    c.multi        = t->world > 1 || t->force_comm;
    c.tiles        = tile_path(t);
    c.sync         = uses_sync(t);
    // pass A split into boundary + interior launches so that the exchange starts after 4 planes per face instead of after
    // the whole pass: an extra launch (+6-7 us per iteration in the compute-only timing at N = 4 and 8), worth it only where
    // the slab is so thin that the 3.1 MB face messages cannot hide behind B_int alone (N >= 4 at 256^3, if a face takes the ~65 us that ~60 GB/s per xGMI direction implies)
    // the schedule (results do not depend on it): sobfu_hip_tiled_set_schedule (autotuner, tests) > heuristic
    const bool want_split = t->schedule == 1 ? true : (t->schedule == 2 ? false : (lz.o1 - lz.o0) <= kSplitAMaxPlanes);
    c.split_a = (lz.lo || lz.hi) && c.z.a_hi > c.z.a_lo && want_split;
    c.serial  = t->schedule == 3;
    c.red_mode = (!c.multi || !c.can_converge || c.sync) ? RED_NONE : (t->comm2 ? RED_OWN_COMM : ((c.serial || c.tiles) ? RED_INLINE : RED_COMM_STREAM));
    return c;
}

// the arrays iteration `it` reads and writes
struct IterBufs {
    const float *psi_in, *f_in;
    float *psi_out, *f_out, *nu;
    const uint32_t* prev;  // the late gate: the row of iteration it-2 (null: ungated)
    uint32_t* row;         // this iteration's row
};
static IterBufs iteration_buffers(const LoopCtx& c, int it) {
    sobfu_hip_tiled* t = c.t;
    IterBufs b;
    b.psi_in = t->c_psi[(it - 1) & 1].get(); b.f_in = t->c_f[(it - 1) & 1].get();
    b.psi_out = t->c_psi[it & 1].get(); b.f_out = t->c_f[it & 1].get();
    b.nu   = t->nUb[c.tiles ? (it & 1) : 0];
    b.prev = (it > 2 && c.can_converge) ? t->rows.gate(c.sync) + (size_t) (it - 2) * kSlots : nullptr;
    b.row  = t->rows.local(it);
    return b;
}

// pass A of the z-slab schedules on one or two plane ranges of the owned block; it writes scratch only: never gated
static int pass_a(const LoopCtx& c, int it, int za, int zb, int za2 = 0, int zb2 = 0) {
    const sobfu_hip_tiled* t = c.t;
    const IterBufs b = iteration_buffers(c, it);
    sobfu_hip::PassALaunch L;
    L.pnp = b.f_in; L.pg = t->c_g.get(); L.psi = b.psi_in; L.nU = b.nu; L.w_reg = t->p.w_reg;
    L.X = t->lay.a[0].L; L.Y = t->lay.a[1].L; L.Z = t->lay.a[2].L;
    L.boxes[0] = {c.own[0], c.own[1], c.own[2], c.own[3], za, zb, false};
    L.boxes[1] = {c.own[0], c.own[1], c.own[2], c.own[3], za2, zb2, false};
    L.n_boxes  = 2;
    L.compact  = true;
    return sobfu_hip::launch_pass_a(L, c.st);
}

// pass B on one or two plane ranges: the owned block with its z shells (extra planes of the march); the one-cell x / y shells are
// direct boxes
static int pass_b(const LoopCtx& c, int it, int za, int zb, int za2 = 0, int zb2 = 0, bool shells = false) {
    const sobfu_hip_tiled* t = c.t;
    const IterBufs b = iteration_buffers(c, it);
    const sobfu_hip::AxisLay &lx = t->lay.a[0], &ly = t->lay.a[1];
    const int ax0 = c.own[0], ax1 = c.own[1], ay0 = c.own[2], ay1 = c.own[3], lo = c.own[4], hi = c.own[5], dbg = t->debug_skip;
    const bool ysh = shells && !(dbg & sobfu_hip::kSkipYShells), xsh = shells && !(dbg & sobfu_hip::kSkipXShells);
    sobfu_hip::PassBLaunch L;
    L.nU = b.nu; L.psi = const_cast<float*>(b.psi_in); L.psi_out = b.psi_out; L.phi_n = t->c_n.get(); L.pnp = b.f_out; L.slots = b.row;
    L.taps = t->taps; L.alpha = t->p.alpha;
    L.X = lx.L; L.Y = ly.L; L.Z = t->lay.a[2].L;
    L.pX = t->X; L.pY = t->Y; L.pZ = t->Z;
    for (int i = 0; i < 6; ++i) L.own[i] = c.own[i];
    L.boxes[0] = {ax0, ax1, ay0, ay1, za, (dbg & sobfu_hip::kSkipOwnedB) ? za : zb, false};
    L.boxes[1] = {ax0, ax1, ay0, ay1, za2, zb2, false};
    L.boxes[2] = {ax0, ax1, ay0 - 1, (ysh && ly.lo) ? ay0 : ay0 - 1, lo, hi, true};
    L.boxes[3] = {ax0, ax1, ay1, (ysh && ly.hi) ? ay1 + 1 : ay1, lo, hi, true};
    L.boxes[4] = {ax0 - 1, (xsh && lx.lo) ? ax0 : ax0 - 1, ay0, ay1, lo, hi, true};
    L.boxes[5] = {ax1, (xsh && lx.hi) ? ax1 + 1 : ax1, ay0, ay1, lo, hi, true};
    L.n_boxes  = 6;
    L.prev_slots = b.prev; L.max_update_norm = t->p.max_update_norm; L.prev_rows = it > 3 ? 2 : 1;
    L.compact     = true;
    L.sys_acquire = c.sync;  // direct transport (and the handles that time its launches): peer-written cells are read at system scope
    return sobfu_hip::launch_pass_b(L, c.st);
}

// row it-2 must be global before the first pass-B launch of iteration `it`: an asynchronous reduce of the latest row of this parity is
// behind ev_red[parity]
static int wait_gate(const LoopCtx& c, int it) {
    sobfu_hip_tiled* t = c.t;
    if (it > 2 && c.can_converge && t->q.red_issued[it & 1]) SOBFU_HIP_TRY(hipStreamWaitEvent(c.st, t->ev_red[it & 1].get(), 0));
    return 0;
}

// row `it` is complete on the loop's stream; it gates iteration it+2
static int after_b(const LoopCtx& c, int it) {
    sobfu_hip_tiled* t          = c.t;
    sobfu_hip_tiled::Session& q = t->q;
    if (it > q.cap - 2) return 0;  // rows past cap - 2 gate nothing: the tail rows are reduced once, by tiled_end
    // every row after the last one reduced so far, up to this one (normally just this one; more after a change of schedule
    // in mid-solve, whose reduction points differ)
    const int first  = std::min(q.red_upto + 1, it);
    const size_t cnt = (size_t) (it - first + 1) * kSlots;
    if (c.red_mode == RED_INLINE) {
        SOBFU_TRY(allreduce_max(t, t->rows.local(first), cnt, c.st));
        q.red_upto = it;
    }
    if (c.red_mode == RED_OWN_COMM) {
        SOBFU_HIP_TRY(hipEventRecord(t->ev_row.get(), c.st));
        SOBFU_HIP_TRY(hipStreamWaitEvent(t->red_stream.get(), t->ev_row.get(), 0));
        SOBFU_TRY(allreduce_max(t, t->rows.local(first), cnt, t->red_stream.get(), true));
        SOBFU_HIP_TRY(hipEventRecord(t->ev_red[it & 1].get(), t->red_stream.get()));
        q.red_issued[it & 1] = true;
        q.red_upto = it;
    }
    return 0;
}

// the tail of every schedule, behind the last pass-B launch of iteration `it`
static int finish_iteration(const LoopCtx& c, int it) {
    sobfu_hip_tiled* t = c.t;
    SOBFU_TRY(after_b(c, it));
    t->q.launched = it;  // advanced once the iteration is fully enqueued
    if (t->comm && !t->first_checked) SOBFU_TRY(first_iteration_watchdog(t, c.st));
    return 0;
}

// Timing of a sampled iteration's three pieces (sobfu_hip_tiled_set_profiling; tile path and serial schedule, whole iterations only):
// four events on the loop's stream -- 0 | pass A | 1 | exchange | 2 | pass B | 3.
struct ProfSample {
    sobfu_hip_tiled* t;
    hipStream_t st;
    bool on;
    ProfSample(const LoopCtx& c, int it) : t(c.t), st(c.st) {
        on = (c.tiles || c.serial) && c.phases == 3 && t->prof_stride > 0 && it % t->prof_stride == 0 && (size_t) 4 * (t->prof_pending + 1) <= t->prof_ev.size();
    }
    int mark(int k) {
        if (!on) return 0;
        SOBFU_HIP_TRY(hipEventRecord(t->prof_ev[4 * t->prof_pending + k].get(), st));
        if (k == 3) t->prof_pending += 1;
        return 0;
    }
};

// TILE PATH -- pass A's launch carries the exchange (push boxes first).  Direct transport: that is all of it -- the
// launch retires when the neighbours' cells have landed too.  RCCL / callback: the packed buffer travels, one
// kernel scatters what arrived.  No cross-stream events anywhere.
static int issue_tile(const LoopCtx& c, int it) {
    sobfu_hip_tiled* t = c.t;
    const IterBufs b   = iteration_buffers(c, it);
    const int dbg      = t->debug_skip;
    ProfSample prof(c, it);
    if (c.phases & 1) {
        SOBFU_TRY(prof.mark(0));
        const bool pushes        = (c.multi || c.sync) && !(dbg & sobfu_hip::kSkipPushBoxes);  // a world of one has no messages
        const uint32_t* row_prev = (c.sync && it >= 2) ? t->rows.local(it - 1) : nullptr;
        if (!(dbg & sobfu_hip::kSkipPassA))
            SOBFU_TRY(sobfu_hip::launch_tile_pass_a_plan((pushes ? t->a_plan[it & 1] : t->a_own_plan).get(), b.f_in, t->c_g.get(), b.psi_in, b.nu, t->p.w_reg,
                                                         c.sync ? t->sync_d.get() : nullptr, t->q.seq_base + (uint32_t) it, t->wait_enabled, row_prev,
                                                         (uint32_t) (it - 1), c.st));
        SOBFU_TRY(prof.mark(1));
        if (c.multi && !c.sync) SOBFU_TRY(exchange_packed(t, b.nu, c.st));
    }
    if (c.phases & 2) {
        SOBFU_TRY(wait_gate(c, it));
        SOBFU_TRY(prof.mark(2));
        if (!(dbg & sobfu_hip::kSkipPassB)) SOBFU_TRY(pass_b(c, it, c.z.b_first, c.z.b_last, 0, 0, !(dbg & sobfu_hip::kSkipShells)));
        SOBFU_TRY(prof.mark(3));
        SOBFU_TRY(finish_iteration(c, it));
    }
    return 0;
}

// SERIAL z-slab schedule -- no overlap, no cross-stream events: pass A, the exchange and pass B in line on the loop's stream.  Every
// event record / wait between two kernels costs a few microseconds of drained pipeline (~20 us per iteration for the overlapped
// schedule's three), which a fast exchange on a thin slab does not repay.
static int issue_slab_serial(const LoopCtx& c, int it) {
    sobfu_hip_tiled* t = c.t;
    ProfSample prof(c, it);
    SOBFU_TRY(prof.mark(0));
    SOBFU_TRY(pass_a(c, it, c.own[4], c.own[5]));
    SOBFU_TRY(prof.mark(1));
    if (c.multi) SOBFU_TRY(exchange_planes(t, iteration_buffers(c, it).nu, kHalo, c.st));
    SOBFU_TRY(wait_gate(c, it));
    SOBFU_TRY(prof.mark(2));
    SOBFU_TRY(pass_b(c, it, c.z.b_first, c.z.b_last));
    SOBFU_TRY(prof.mark(3));
    return finish_iteration(c, it);
}

// OVERLAPPED z-slab schedule (the drawing at the top of the file):
//     A_bnd  ->  ev_bnd  ->  [comm stream] exchange (+ the reduction of row it-1)  ->  ev_xchg
//     A_int, B_int                                  ... run while the exchange is in flight
//     wait(ev_xchg)  ->  B_bnd
static int issue_slab_overlapped(const LoopCtx& c, int it) {
    sobfu_hip_tiled* t          = c.t;
    sobfu_hip_tiled::Session& q = t->q;
    const sobfu_hip::PlaneRanges& z = c.z;
    const int lo = c.own[4], hi = c.own[5];
    // both boundary regions of a pass go out as ONE launch (two plane ranges)
    if (c.split_a) SOBFU_TRY(pass_a(c, it, lo, z.a_lo, z.a_hi, hi));
    else SOBFU_TRY(pass_a(c, it, lo, hi));
    if (c.multi) {
        SOBFU_HIP_TRY(hipEventRecord(t->ev_bnd.get(), c.st));
        SOBFU_HIP_TRY(hipStreamWaitEvent(t->comm_stream.get(), t->ev_bnd.get(), 0));
        SOBFU_TRY(exchange_planes(t, iteration_buffers(c, it).nu, kHalo, t->comm_stream.get()));
        SOBFU_HIP_TRY(hipEventRecord(t->ev_xchg.get(), t->comm_stream.get()));
        if (c.red_mode == RED_COMM_STREAM && it >= 2 && it < q.cap && q.red_upto < it - 1) {
            // row it-1 is complete (its pass B precedes this iteration's ev_bnd, which the comm stream has waited for) and
            // gates iteration it+1: reduce it (and any earlier row not reduced yet) behind this iteration's exchange
            const int first = q.red_upto + 1;
            SOBFU_TRY(allreduce_max(t, t->rows.local(first), (size_t) (it - first) * kSlots, t->comm_stream.get()));
            SOBFU_HIP_TRY(hipEventRecord(t->ev_red[(it - 1) & 1].get(), t->comm_stream.get()));
            q.red_issued[(it - 1) & 1] = true;
            q.red_upto = it - 1;
        }
    }
    if (c.split_a && z.a_hi > z.a_lo) SOBFU_TRY(pass_a(c, it, z.a_lo, z.a_hi));
    SOBFU_TRY(wait_gate(c, it));
    if (z.b_hi > z.b_lo) SOBFU_TRY(pass_b(c, it, z.b_lo, z.b_hi));
    // the next iteration's A_bnd overwrites nabla_U planes the exchange of THIS iteration sent: it runs on the loop's stream after
    // this wait, so the sends have completed by then; the next exchange's receives overwrite halo planes B_bnd
    // of THIS iteration read: the comm stream starts it only after the next ev_bnd, recorded on the loop's stream behind B_bnd
    if (c.multi) SOBFU_HIP_TRY(hipStreamWaitEvent(c.st, t->ev_xchg.get(), 0));
    if (z.b_lo > z.b_first || z.b_last > z.b_hi) SOBFU_TRY(pass_b(c, it, z.b_first, z.b_lo, z.b_hi, z.b_last));
    return finish_iteration(c, it);
}

// enqueues iterations launched+1 .. launched+n_steps (phases: see LoopCtx)
static int tiled_step_impl(sobfu_hip_tiled* t, int n_steps, hipStream_t st, int phases) {
    sobfu_hip_tiled::Session& q = t->q;
    if (!q.active || n_steps < 0 || q.launched + n_steps > q.cap) return SOBFU_E_BADARG;
    if (t->dead) return SOBFU_E_TIMEOUT;
    const LoopCtx c     = loop_context(t, st, phases);
    const auto host_t0  = std::chrono::steady_clock::now();
    const int last      = q.launched + n_steps;
    for (int it = q.launched + 1; it <= last; ++it) {
        if (c.tiles) SOBFU_TRY(issue_tile(c, it));
        else if (phases != 3) return SOBFU_E_UNSUPPORTED;  // a slab schedule is not stepped by phase
        else if (c.serial) SOBFU_TRY(issue_slab_serial(c, it));
        else SOBFU_TRY(issue_slab_overlapped(c, it));
    }
    if (n_steps > 0)
        t->last_enqueue_us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - host_t0).count() / n_steps;
    return 0;
}

// an error inside the loop: peers may be blocked in a collective this rank never issued -- drain what was enqueued, abort the
// communicators (so that the peers' calls return instead of hanging) and give the handle up
static int tiled_step(sobfu_hip_tiled* t, int n_steps, hipStream_t st, int phases = 3) {
    const int rc = tiled_step_impl(t, n_steps, st, phases);
    if (rc != 0 && rc != SOBFU_E_BADARG && rc != SOBFU_E_UNSUPPORTED) {
        abort_comms(t);  // FIRST: the stream may hold an RCCL kernel waiting for a peer this rank will never answer; the abort releases it
        (void) hipStreamSynchronize(st);
        t->q.active = false;
    }
    return rc;
}

// direct transport, end of a solve: the last max-norm row travels now; the handshake also tells every rank that its neighbours
// have retired their last pass B, i.e. that the next solve's first pushes cannot land under a kernel still reading the halo cells
static int tiled_flush(sobfu_hip_tiled* t, hipStream_t st) {
    sobfu_hip_tiled::Session& q = t->q;
    if (q.flushed) return 0;
    const int n = q.launched;
    const uint32_t seq = q.seq_base + (uint32_t) n + 1u;
    SOBFU_TRY(sobfu_hip::launch_tile_flush(t->sync_d.get(), seq, t->wait_enabled, n > 0 ? t->rows.local(n) : nullptr, (uint32_t) n, st));
    t->seq_total = seq;
    q.flushed    = true;
    return 0;
}

static int tiled_end(sobfu_hip_tiled* t, sobfu_hip_solver_report* report, float* per_iter_max_norm, hipStream_t st) {
    sobfu_hip_tiled::Session& q = t->q;
    if (!q.active) return SOBFU_E_BADARG;
    if (t->dead) return SOBFU_E_TIMEOUT;
    const sobfu_hip_solver_params& p = t->p;
    sobfu_hip_solver_report r{};
    r.last_max_update_norm = r.last_max_update_index = r.last_e_data = r.last_e_reg = NAN;
    const LoopCtx c   = loop_context(t, st, 3);
    const int n_iters = q.launched;
    if (c.sync) {
        SOBFU_TRY(tiled_flush(t, st));
    } else if (c.multi && n_iters > 0) {  // rows the loop has not reduced yet: all of them without a threshold, the tail otherwise
        for (int k = 0; k < 2; ++k)
            if (q.red_issued[k]) SOBFU_HIP_TRY(hipStreamWaitEvent(st, t->ev_red[k].get(), 0));
        const int first = q.red_upto + 1;
        if (first <= n_iters) SOBFU_TRY(allreduce_max(t, t->rows.local(first), (size_t) (n_iters - first + 1) * kSlots, st));
    }
    std::vector<uint32_t> hs((size_t) std::max(n_iters, 1) * kSlots, 0u);
    if (n_iters > 0) SOBFU_HIP_TRY(hipMemcpyAsync(hs.data(), t->rows.gate(c.sync) + kSlots, (size_t) n_iters * kSlots * 4, hipMemcpyDeviceToHost, st));
    SOBFU_HIP_TRY(hipStreamSynchronize(st));
    if (c.sync) {
        uint32_t err = 0;
        SOBFU_HIP_TRY(hipMemcpy(&err, &t->sync_d->err, 4, hipMemcpyDeviceToHost));
        if (err) {
            std::fprintf(stderr, "sobfu_hip: rank %d: the arrival flag of rank %u did not reach this GPU within the deadline (direct transport)\n",
                         t->rank, err - 1u);
            t->dead  = true;
            q.active = false;
            return SOBFU_E_TIMEOUT;
        }
    }
    int done = n_iters;
    for (int k = 0; k < n_iters; ++k) {
        const float v = sobfu_hip::slots_to_norm(hs.data() + (size_t) k * kSlots);
        if (per_iter_max_norm) per_iter_max_norm[k] = v;
        r.last_max_update_norm = v;
        if (c.can_converge && v <= p.max_update_norm) {  // solver.cu:183 -- iteration k+2 ran speculatively, later ones not at all
            done = k + 1;
            r.converged = 1;
            break;
        }
    }
    r.iterations = done;
    // leave the compact format from the half that holds the state after `done` iterations: psi.xyz back,
    // phi_n o psi = apply(phi_n, psi) (the state of solver.cu:168)
    SOBFU_TRY(sobfu_hip::launch_unpack_vec(t->c_psi[done & 1].get(), q.psi, t->NL, st));
    SOBFU_TRY(sobfu_hip_tile3_apply(q.pn, t->X, t->Y, t->Z, q.pnp, q.psi, t->lay.a[0].L, t->lay.a[1].L, t->lay.a[2].L, st));
    SOBFU_HIP_TRY(hipStreamSynchronize(st));
    q.active = false;
    if (report) *report = r;
    return 0;
}

int sobfu_hip_tiled_begin(sobfu_hip_tiled* t, const float* d_phi_global_local, const float* d_phi_n_full, float* d_phi_n_psi_local,
                          float* d_psi_local, int max_iters, void* stream) {
    SOBFU_CHECK_ARGS(t && d_phi_global_local && d_phi_n_full && d_phi_n_psi_local && d_psi_local && max_iters >= 0);
    return tiled_begin(t, d_phi_global_local, d_phi_n_full, d_phi_n_psi_local, d_psi_local, max_iters, (hipStream_t) stream);
}

int sobfu_hip_tiled_step(sobfu_hip_tiled* t, int n_iters, void* stream) {
    SOBFU_CHECK_ARGS(t && n_iters >= 0);
    return tiled_step(t, n_iters, (hipStream_t) stream);
}

int sobfu_hip_tiled_step_phase(sobfu_hip_tiled* t, int phase, void* stream) {
    SOBFU_CHECK_ARGS(t && phase >= 0 && phase <= 2);
    if (phase == 2) return (t->q.active && uses_sync(t)) ? tiled_flush(t, (hipStream_t) stream) : SOBFU_E_BADARG;
    return tiled_step(t, 1, (hipStream_t) stream, phase == 0 ? 1 : 2);
}

int sobfu_hip_tiled_end(sobfu_hip_tiled* t, sobfu_hip_solver_report* report, float* per_iter_max_norm, void* stream) {
    SOBFU_CHECK_ARGS(t);
    return tiled_end(t, report, per_iter_max_norm, (hipStream_t) stream);
}

int sobfu_hip_tiled_iterate(sobfu_hip_tiled* t, const float* d_phi_global_local, const float* d_phi_n_full,
                            float* d_phi_n_psi_local, float* d_psi_local, int n_iters, sobfu_hip_solver_report* report,
                            float* per_iter_max_norm, void* stream) {
    SOBFU_CHECK_ARGS(t && d_phi_global_local && d_phi_n_full && d_phi_n_psi_local && d_psi_local && n_iters >= 0);
    hipStream_t st = (hipStream_t) stream;
    SOBFU_TRY(tiled_begin(t, d_phi_global_local, d_phi_n_full, d_phi_n_psi_local, d_psi_local, n_iters, st));
    SOBFU_TRY(tiled_step(t, n_iters, st));
    return tiled_end(t, report, per_iter_max_norm, st);
}

}  // extern "C"
