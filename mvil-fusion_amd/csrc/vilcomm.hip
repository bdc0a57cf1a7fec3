// vilcomm.hip -- the multi-GPU exchange of libvilsolve.so (vil_comm.hpp): the three transports, the packed "slim" message, their kernels.
#include <cstring>
#include <pthread.h>
#include <dlfcn.h>
#include <rccl/rccl.h>   // types only: RCCL is bound at run time (dlopen) so that a process which already
                         // carries an RCCL (PyTorch bundles one) never ends up with two copies
#include "vil_comm.hpp"
namespace {
struct RcclApi {
    void* h = nullptr;
    ncclResult_t (*GetUniqueId)(ncclUniqueId*) = nullptr;
    ncclResult_t (*CommInitRank)(ncclComm_t*, int, ncclUniqueId, int) = nullptr;
    ncclResult_t (*AllReduce)(const void*, void*, size_t, ncclDataType_t, ncclRedOp_t, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*AllGather)(const void*, void*, size_t, ncclDataType_t, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
    bool load() {
        if (h) return true;
        const char* names[] = {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"};
        for (const char* n : names) { h = dlopen(n, RTLD_NOW | RTLD_NOLOAD); if (h) break; }     // reuse a copy that is already mapped
        if (!h) for (const char* n : names) { h = dlopen(n, RTLD_NOW | RTLD_GLOBAL); if (h) break; }
        if (!h) return false;
        GetUniqueId = (decltype(GetUniqueId))dlsym(h, "ncclGetUniqueId");
        CommInitRank = (decltype(CommInitRank))dlsym(h, "ncclCommInitRank");
        AllReduce = (decltype(AllReduce))dlsym(h, "ncclAllReduce");
        AllGather = (decltype(AllGather))dlsym(h, "ncclAllGather");
        CommDestroy = (decltype(CommDestroy))dlsym(h, "ncclCommDestroy");
        return GetUniqueId && CommInitRank && AllReduce && AllGather && CommDestroy;
    }
};
RcclApi g_rccl;      // one per process
}  // namespace

// In-process communicator: the contexts of ONE process (one host thread each) sum their buffers through device
// memory.  Same call sites and the same deterministic result on every rank as the RCCL path; used where the ranks share
// a process, and by the tests to run a sharded solve on a single device.
struct LocalComm {
    int n = 0;
    pthread_barrier_t bar;
    double* ptr[8] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    int err[8] = {0, 0, 0, 0, 0, 0, 0, 0};        // per-rank status of the current collective: an error on one rank is an error on all (nobody is left at a barrier)
    ~LocalComm() { if (n) pthread_barrier_destroy(&bar); }
    // every rank posts its status, waits, and reads the worst one: collective error exits
    int agree(int rank, int st) { err[rank] = st; pthread_barrier_wait(&bar); int w = 0; for (int r = 0; r < n; ++r) w = std::min(w, err[r]); pthread_barrier_wait(&bar); return w; }
};
struct PeerPtrs { const double* p[8]; int n; };

// Multi-process exchange without RCCL (the per-iteration message is latency-bound; on the fully connected xGMI mesh a one-shot
// "everybody writes to everybody, then sums locally" beats a ring): every rank owns an INBOX in its device memory -- world x 2 (parity of
// the collective's sequence number) x cap doubles, then one flag per (source rank, parity), 64 bytes apart -- exported with hipIpcGetMemHandle
// and opened by every peer.  A collective = k_ipc_push (my message into every inbox, a system-scope fence, then the flags) ->
// k_ipc_wait (one workgroup spins until every source's flag carries the sequence number) -> k_ipc_sum (rank order: identical bits on every
// rank).  Everything is in stream order and the sequence number lives in device memory: capturable in a hipGraph, nothing for the host to wait for.
// Two parities suffice: a peer can only push collective i + 2 after it has summed i + 1, which needs MY push of i + 1, which I do after my sum of i.
struct IpcComm {
    int world = 0, rank = 0; size_t cap = 0;
    bool ready = false;                       // every peer's handle is open (vil_comm_ipc_init): before that a collective would write through null inbox pointers
    char* base = nullptr;                     // my allocation: [inbox | flags | seq | count]
    void* peer_base[8] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};      // opened handles (my own: base)
    size_t off_flags = 0, off_seq = 0;
    double* inbox(int r) const { return (double*)peer_base[r]; }
    int* flags(int r) const { return (int*)((char*)peer_base[r] + off_flags); }
    int* seq() const { return (int*)(base + off_seq); }
};
struct IpcPtrs { double* inbox[8]; int* flags[8]; int world, rank; size_t cap; int* seq; int* count; };
// sym = D > 0: the message starts with a symmetric D x D block (the reduced system S', both triangles filled with the same bits by the gather): only
// its lower triangle travels, the sum writes both mirror images -- identical bits, D (D - 1) / 2 doubles less per rank pair (98 of 484 kB at K = 10)
__device__ __forceinline__ bool sym_skip(size_t e, int sym) { if (!sym || e >= (size_t)sym * sym) return false; const int i = (int)(e / sym), j = (int)(e - (size_t)i * sym); return j > i; }
__device__ __forceinline__ void sym_store(double* out, size_t e, int sym, double v) {
    out[e] = v;
    if (sym && e < (size_t)sym * sym) { const int i = (int)(e / sym), j = (int)(e - (size_t)i * sym); if (j < i) out[(size_t)j * sym + i] = v; }
}
__device__ __forceinline__ int seg_owner(const OwnSeg& S, size_t e) {          // -1: summed over all ranks (OwnSeg: vil_comm.hpp)
    if (S.n == 0 || e < S.cam) return -1;
    const size_t a = e - S.cam, Lp = (size_t)S.Lp;
    const bool lm = a < 17 * Lp;
    const int v = a < 4 * Lp ? (int)(a % Lp) : (lm ? (int)((a - 4 * Lp) / 13) : (int)((a - 17 * Lp) / 6));
    const int* b = lm ? S.lb : S.fb;
    int r = 0;
    while (r + 1 < S.n && v >= b[r + 1]) ++r;
    return r;
}
__global__ void k_ipc_push(const double* send, size_t cnt, IpcPtrs I, int sym, OwnSeg S) {
    const int sq = *I.seq + 1, par = sq & 1;
    const size_t off = ((size_t)I.rank * 2 + par) * I.cap;
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < cnt; e += (size_t)gridDim.x * blockDim.x) {
        if (sym_skip(e, sym)) continue;
        const int own = seg_owner(S, e);
        if (own >= 0 && own != I.rank) continue;          // somebody else's landmark: zero here, nothing to send
        const double v = send[e];
        for (int r = 0; r < I.world; ++r) I.inbox[r][off + e] = v;
    }
    __threadfence_system();                   // this thread's stores have reached every peer ...
    __syncthreads();
    __shared__ int last;
    if (threadIdx.x == 0) last = atomicAdd(I.count, 1) == (int)gridDim.x - 1;
    __syncthreads();
    if (last && threadIdx.x == 0) {           // ... all blocks' have: the flags go out, the sequence number advances
        __threadfence_system();
        *I.count = 0;
        for (int r = 0; r < I.world; ++r) __hip_atomic_store(I.flags[r] + 16 * (I.rank * 2 + par), sq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
        *I.seq = sq;
    }
}
__global__ void k_ipc_wait(IpcPtrs I) {
    const int sq = *I.seq, par = sq & 1, t = threadIdx.x;       // (k_ipc_push of this collective has advanced it: same stream)
    if (t < I.world) while (__hip_atomic_load(I.flags[I.rank] + 16 * (t * 2 + par), __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_SYSTEM) != sq) __builtin_amdgcn_s_sleep(8);
}
__global__ void k_ipc_sum(double* out, size_t cnt, IpcPtrs I, int sym, OwnSeg S) {
    const int par = *I.seq & 1;
    const double* in = I.inbox[I.rank];
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < cnt; e += (size_t)gridDim.x * blockDim.x) {
        if (sym_skip(e, sym)) continue;
        const int own = seg_owner(S, e);
        double s = 0;
        if (own >= 0) s = __builtin_nontemporal_load(in + ((size_t)own * 2 + par) * I.cap + e);                        // the owner's entry (everybody else's is zero and did not travel)
        else for (int r = 0; r < I.world; ++r) s += __builtin_nontemporal_load(in + ((size_t)r * 2 + par) * I.cap + e);      // written by peers: not through a stale cache line
        sym_store(out, e, sym, s);
    }
}
__global__ void k_sum_peers(double* out, PeerPtrs pp, size_t cnt, int sym, OwnSeg S) {
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < cnt; e += (size_t)gridDim.x * blockDim.x) {
        if (sym_skip(e, sym)) continue;
        const int own = seg_owner(S, e);
        double s = 0;
        if (own >= 0) s = pp.p[own][e];
        else for (int r = 0; r < pp.n; ++r) s += pp.p[r][e];     // rank order: identical bits on every rank
        sym_store(out, e, sym, s);
    }
}

// The same slim message for RCCL ("[upper(S), g, cost]", ~100 kB): the per-iteration set is PACKED into M = [lower triangle of S' | g, b_c, diag | cost]
// (D (D + 1) / 2 + 3 D + 4 doubles, summed by ONE ncclAllReduce) and G = this rank's slice of the landmark arrays [h_ll, b_l, 1/pivot, scale | e_A | e_O], padded
// to the largest slice (ONE ncclAllGather: a landmark's entries live on its owner only, so the sum over ranks is the owner's value -- nothing to add), and
// UNPACKED into set 1 with both mirror images of S'.  At K = 10 / 1000 landmarks / world 8 RCCL moves 103 + 48 kB per rank instead of all-reducing 484 kB.
// staging (doubles): [M camS | G gmax | Msum camS | Gall world x gmax]; pack / unpack do not know the transport -- the tests run them over the in-process
// communicator with k_slim_emul standing in for the two RCCL calls (vil_debug_set_slim_emul), on 2 / 3 / 8 ranks of one device.
struct SlimLay { int D, Lp, n, rank; size_t cam, camS, gmax, span; int lb[9], fb[9]; };
__device__ __forceinline__ size_t slim_tri(int i, int j) { return (size_t)i * (i + 1) / 2 + j; }
// position of set entry e (e >= cam) inside its owner's slice; *owner receives the rank
__device__ __forceinline__ size_t slim_slot(const SlimLay& Y, size_t e, int* owner) {
    const size_t a = e - Y.cam, Lp = (size_t)Y.Lp;
    const bool lm = a < 17 * Lp;
    const int v = a < 4 * Lp ? (int)(a % Lp) : (lm ? (int)((a - 4 * Lp) / 13) : (int)((a - 17 * Lp) / 6));
    const int* b = lm ? Y.lb : Y.fb;
    if (v >= b[Y.n]) { *owner = -1; return 0; }      // padding of an empty array (Lp = max(L, 1), Fp = max(n_vis, 1) with L or n_vis = 0): nobody owns it, it stays zero
    int r = 0;
    while (r + 1 < Y.n && v >= b[r + 1]) ++r;
    *owner = r;
    const size_t nL = (size_t)(Y.lb[r + 1] - Y.lb[r]);
    if (a < 4 * Lp) return (a / Lp) * nL + (size_t)(v - Y.lb[r]);
    if (lm) return 4 * nL + (a - 4 * Lp) - 13 * (size_t)Y.lb[r];
    return 17 * nL + (a - 17 * Lp) - 6 * (size_t)Y.fb[r];
}
__global__ void k_slim_pack(const double* set0, double* M, double* G, SlimLay Y) {
    const size_t DD = (size_t)Y.D * Y.D, trin = (size_t)Y.D * (Y.D + 1) / 2;
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < Y.span; e += (size_t)gridDim.x * blockDim.x) {
        if (e < DD) { const int i = (int)(e / Y.D), j = (int)(e - (size_t)i * Y.D); if (j <= i) M[slim_tri(i, j)] = set0[e]; }
        else if (e < Y.cam) M[trin + (e - DD)] = set0[e];
        else { int r; const size_t g = slim_slot(Y, e, &r); if (r == Y.rank) G[g] = set0[e]; }
    }
}
__global__ void k_slim_unpack(double* set1, const double* Msum, const double* Gall, SlimLay Y) {
    const size_t DD = (size_t)Y.D * Y.D, trin = (size_t)Y.D * (Y.D + 1) / 2;
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < Y.span; e += (size_t)gridDim.x * blockDim.x) {
        double v;
        if (e < DD) { const int i = (int)(e / Y.D), j = (int)(e - (size_t)i * Y.D); v = Msum[slim_tri(max(i, j), min(i, j))]; }
        else if (e < Y.cam) v = Msum[trin + (e - DD)];
        else { int r; const size_t g = slim_slot(Y, e, &r); v = r >= 0 ? Gall[(size_t)r * Y.gmax + g] : 0.0; }
        set1[e] = v;
    }
}
// stand-in for ncclAllReduce(M -> Msum) + ncclAllGather(G -> Gall) over the in-process communicator (tests): pp.p[r] = rank r's staging buffer
__global__ void k_slim_emul(double* Msum, double* Gall, PeerPtrs pp, SlimLay Y) {
    const size_t tot = Y.camS + (size_t)pp.n * Y.gmax;
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < tot; e += (size_t)gridDim.x * blockDim.x) {
        if (e < Y.camS) { double a = 0; for (int r = 0; r < pp.n; ++r) a += pp.p[r][e]; Msum[e] = a; }
        else { const size_t q = e - Y.camS; const int r = (int)(q / Y.gmax); Gall[q] = pp.p[r][Y.camS + (q - (size_t)r * Y.gmax)]; }
    }
}

static const OwnSeg kNoSeg = {0, 0, 0, {0}, {0}};
static SlimLay slim_layout(const OwnSeg& S, int rank, int D, size_t span) {
    SlimLay Y; memset(&Y, 0, sizeof Y);
    Y.D = D; Y.Lp = S.Lp; Y.n = S.n; Y.rank = rank; Y.cam = S.cam; Y.span = span;
    Y.camS = ((size_t)Y.D * (Y.D + 1) / 2 + (S.cam - (size_t)Y.D * Y.D) + 1) & ~size_t(1);
    for (int r = 0; r <= S.n; ++r) { Y.lb[r] = S.lb[r]; Y.fb[r] = S.fb[r]; }
    for (int r = 0; r < S.n; ++r) Y.gmax = std::max(Y.gmax, (size_t)17 * (S.lb[r + 1] - S.lb[r]) + (size_t)6 * (S.fb[r + 1] - S.fb[r]));
    Y.gmax = (Y.gmax + 2) & ~size_t(1);
    return Y;
}
// One exchange of the in-process communicator: synchronise, publish my buffer, agree, launch(every rank's buffer), synchronise, agree.  Every HIP failure
// (st: the caller's so far) is carried to the next agreement point instead of returning past a barrier the other ranks wait at.
template <class Launch> static int local_exchange(LocalComm* lc, int rank, hipStream_t stream, const double* mine, int st, Launch launch) {
    if (hipStreamSynchronize(stream) != hipSuccess) st = VIL_ERR_DEVICE;
    lc->ptr[rank] = const_cast<double*>(mine);
    st = lc->agree(rank, st);                             // all buffers are complete and published (or somebody failed)
    if (st != VIL_OK) return st;
    PeerPtrs pp; pp.n = lc->n;
    for (int r = 0; r < 8; ++r) pp.p[r] = r < lc->n ? lc->ptr[r] : nullptr;
    launch(pp);
    if (hipStreamSynchronize(stream) != hipSuccess) st = VIL_ERR_DEVICE;
    return lc->agree(rank, st);                           // every rank has read every buffer
}

int Comm::transport() const { return rccl ? 1 : (local ? 2 : (ipc ? (ipc->ready ? 3 : -3) : 0)); }
void Comm::set_owners(const std::vector<int>& lms, int L, int K) {
    OwnSeg& S = own; memset(&S, 0, sizeof S);
    S.n = world <= 8 ? world : 0; S.Lp = std::max(L, 1);          // (more than eight ranks: RCCL only, which sums the whole set -- n = 0)
    for (int r = 0; r <= S.n; ++r) { S.lb[r] = shard_cut(lms, L, r, world); S.fb[r] = lms[S.lb[r]]; }
    const size_t D = 15 * (size_t)K + 7; S.cam = (D * D + 3 * D + 3 + 1) & ~size_t(1);
}
int Comm::ipc_sum(hipStream_t stream, const double* send, double* recv, size_t cnt, int sym, const OwnSeg& seg) {
    IpcComm* ic = ipc.get();
    if (!ic->ready) return VIL_ERR_COMM;                // vil_comm_ipc_export without vil_comm_ipc_init: the peers' inboxes are not mapped yet
    if (cnt > ic->cap) return VIL_ERR_UNSUPPORTED;      // the inbox was sized at vil_comm_ipc_export
    IpcPtrs I; memset(&I, 0, sizeof I);
    for (int r = 0; r < ic->world; ++r) { I.inbox[r] = ic->inbox(r); I.flags[r] = ic->flags(r); }
    I.world = ic->world; I.rank = ic->rank; I.cap = ic->cap; I.seq = ic->seq(); I.count = ic->seq() + 16;
    const unsigned nb = (unsigned)std::min<size_t>(128, (cnt + 255) / 256);
    hipLaunchKernelGGL(k_ipc_push, dim3(nb), dim3(256), 0, stream, send, cnt, I, sym, seg);
    hipLaunchKernelGGL(k_ipc_wait, dim3(1), dim3(64), 0, stream, I);
    hipLaunchKernelGGL(k_ipc_sum, dim3(nb), dim3(256), 0, stream, recv, cnt, I, sym, seg);
    return VIL_OK;
}
// the per-iteration collective as a packed message: pack -> all-reduce of M + all-gather of the owners' slices -> unpack (see SlimLay)
int Comm::slim_sum(hipStream_t stream, const double* send, double* recv, int D, size_t span) {
    const SlimLay Y = slim_layout(own, rank, D, span);
    const size_t need = 2 * Y.camS + (size_t)(1 + world) * Y.gmax;
    LocalComm* lc = rccl ? nullptr : local.get();
    int st = VIL_OK;
    if (need > slim_buf.cap) {
        if (slim_buf.reserve(need, need) != hipSuccess || hipMemsetAsync(slim_buf.p, 0, 8 * need, stream) != hipSuccess) st = VIL_ERR_DEVICE;
        if (st != VIL_OK && !lc) return st;          // (in-process ranks carry a failure to the agreement point below)
    }
    double* M = slim_buf.p; double* G = M + Y.camS; double* Msum = G + Y.gmax; double* Gall = Msum + Y.camS;
    const unsigned nb = (unsigned)std::min<size_t>(256, (Y.span + 255) / 256);
    if (st == VIL_OK) hipLaunchKernelGGL(k_slim_pack, dim3(nb), dim3(256), 0, stream, send, M, G, Y);
    if (!lc) {
        if (g_rccl.AllReduce(M, Msum, Y.camS, ncclDouble, ncclSum, rccl, stream) != ncclSuccess) return VIL_ERR_COMM;
        if (g_rccl.AllGather(G, Gall, Y.gmax, ncclDouble, rccl, stream) != ncclSuccess) return VIL_ERR_COMM;
    } else if ((st = local_exchange(lc, rank, stream, slim_buf.p, st, [&](const PeerPtrs& pp) {      // every rank's M and G, published as one staging buffer
        hipLaunchKernelGGL(k_slim_emul, dim3(nb), dim3(256), 0, stream, Msum, Gall, pp, Y); })) != VIL_OK) return st;
    hipLaunchKernelGGL(k_slim_unpack, dim3(nb), dim3(256), 0, stream, recv, (const double*)Msum, (const double*)Gall, Y);
    return VIL_OK;
}
int Comm::sum(hipStream_t stream, const double* send, double* recv, size_t cnt, int sym, bool owned_slices, size_t span) {
    const OwnSeg& seg = owned_slices ? own : kNoSeg;
    if (ipc) return ipc_sum(stream, send, recv, cnt, sym, seg);
    if (seg.n > 0 && sym > 0 && cnt == span && slim()) return slim_sum(stream, send, recv, sym, span);
    if (rccl) return g_rccl.AllReduce(send, recv, cnt, ncclDouble, ncclSum, rccl, stream) == ncclSuccess ? VIL_OK : VIL_ERR_COMM;
    if (local) {
        const bool inplace = send == recv;
        int st = inplace && tmp.reserve(cnt, cnt) != hipSuccess ? VIL_ERR_DEVICE : VIL_OK;
        double* out = inplace ? tmp.p : recv;
        st = local_exchange(local.get(), rank, stream, send, st, [&](const PeerPtrs& pp) {
            hipLaunchKernelGGL(k_sum_peers, dim3((unsigned)std::min<size_t>(256, (cnt + 255) / 256)), dim3(256), 0, stream, out, pp, cnt, sym, seg); });
        if (st != VIL_OK) return st;
        if (inplace) HIPCHK(hipMemcpyAsync(recv, tmp.p, 8 * cnt, hipMemcpyDeviceToDevice, stream));
        return VIL_OK;
    }
    if (send != recv) HIPCHK(hipMemcpyAsync(recv, send, 8 * cnt, hipMemcpyDeviceToDevice, stream));     // a single rank (vil_debug_set_split)
    return VIL_OK;
}
int Comm::agree(hipStream_t stream, int st) {
    if (local) return local->agree(rank, st);
    if (ipc) {                                             // every rank's status in its own slot of a world-long message: the worst one wins
        const int w = ipc->world; double* h = agree_h.p; for (int r = 0; r < w; ++r) h[r] = r == ipc->rank ? (double)st : 0.0;
        if (hipMemcpyAsync(agree_d.p, h, 8 * (size_t)w, hipMemcpyHostToDevice, stream) != hipSuccess) return VIL_ERR_DEVICE;
        if (ipc_sum(stream, agree_d.p, agree_d.p + 32, (size_t)w, 0, kNoSeg) != VIL_OK) return VIL_ERR_COMM;
        if (hipMemcpyAsync(h + 32, agree_d.p + 32, 8 * (size_t)w, hipMemcpyDeviceToHost, stream) != hipSuccess) return VIL_ERR_DEVICE;
        if (hipStreamSynchronize(stream) != hipSuccess) return VIL_ERR_DEVICE;
        int worst = 0; for (int r = 0; r < w; ++r) worst = std::min(worst, (int)h[32 + r]);
        return worst;
    }
    if (rccl) {
        int* h = (int*)agree_h.p; int* d = (int*)agree_d.p; *h = st;
        if (hipMemcpyAsync(d, h, sizeof(int), hipMemcpyHostToDevice, stream) != hipSuccess) return VIL_ERR_DEVICE;
        if (g_rccl.AllReduce(d, d, 1, ncclInt, ncclMin, rccl, stream) != ncclSuccess) return VIL_ERR_COMM;
        if (hipMemcpyAsync(h, d, sizeof(int), hipMemcpyDeviceToHost, stream) != hipSuccess) return VIL_ERR_DEVICE;
        if (hipStreamSynchronize(stream) != hipSuccess) return VIL_ERR_DEVICE;
        return *h;
    }
    return st;
}
// bytes this rank sends to EACH peer per trust-region iteration through the library's own exchanges (peer buffers, in-process communicator): the lower
// triangle of S' + the vectors + its own slice of the landmark arrays.  (RCCL all-reduces the whole set: vil_comm_init.)
void Comm::message_bytes(int D_, size_t span, int64_t* bytes_per_peer, int64_t* bytes_full_set) const {
    const OwnSeg& S = own;
    const size_t D = (size_t)D_, cam_sent = S.cam - D * (D - 1) / 2;
    const size_t mine = S.n > 0 ? (size_t)17 * (S.lb[rank + 1] - S.lb[rank]) + (size_t)6 * (S.fb[rank + 1] - S.fb[rank]) : span - S.cam;
    if (slim()) { const SlimLay Y = slim_layout(S, rank, D_, span); if (bytes_per_peer) *bytes_per_peer = (int64_t)(8 * (Y.camS + Y.gmax)); }      // RCCL: M all-reduced + this rank's padded slice all-gathered
    else if (rccl && world > 1) { if (bytes_per_peer) *bytes_per_peer = (int64_t)(8 * span); }      // RCCL beyond eight ranks: the whole set is all-reduced
    else if (bytes_per_peer) *bytes_per_peer = (int64_t)(8 * (cam_sent + mine));
    if (bytes_full_set) *bytes_full_set = (int64_t)(8 * span);
}
void Comm::release(int device) {
    hipSetDevice(device);
    if (rccl && g_rccl.CommDestroy) g_rccl.CommDestroy(rccl);
    rccl = nullptr; local.reset();
    if (ipc) { for (int r = 0; r < ipc->world; ++r) if (r != ipc->rank && ipc->peer_base[r]) hipIpcCloseMemHandle(ipc->peer_base[r]); hipFree(ipc->base); ipc.reset(); }
    tmp.release(); slim_buf.release();
    agree_h.release(); agree_d.release();
}
int Comm::alloc_agree() { HIPCHK(agree_h.reserve(64, 64)); HIPCHK(agree_d.reserve(64, 64)); return VIL_OK; }
int Comm::unique_id(void* id128) {
    if (!g_rccl.load()) return VIL_ERR_COMM;
    ncclUniqueId id;
    if (g_rccl.GetUniqueId(&id) != ncclSuccess) return VIL_ERR_COMM;
    memcpy(id128, id.internal, NCCL_UNIQUE_ID_BYTES);
    return VIL_OK;
}
int Comm::use_rccl(int device, const void* id128, int rank_, int world_) {
    release(device);
    ncclUniqueId id; memcpy(id.internal, id128, NCCL_UNIQUE_ID_BYTES);
    if (!g_rccl.load()) return VIL_ERR_COMM;
    if (alloc_agree() != VIL_OK) return VIL_ERR_DEVICE;
    if (g_rccl.CommInitRank(&rccl, world_, id, rank_) != ncclSuccess) { rccl = nullptr; return VIL_ERR_COMM; }
    rank = rank_; world = world_;
    return VIL_OK;
}
// multi-process peer-buffer exchange: export the inbox, gather the handles (the launcher's job: torch.distributed / MPI / a pipe), import
int Comm::export_ipc(int device, int rank_, int world_, size_t max_doubles, void* handle64) {
    release(device);
    if (alloc_agree() != VIL_OK) return VIL_ERR_DEVICE;
    auto ic = std::make_shared<IpcComm>();
    ic->world = world_; ic->rank = rank_; ic->cap = (max_doubles + 31) & ~size_t(31);
    ic->off_flags = 8 * (size_t)world_ * 2 * ic->cap; ic->off_seq = ic->off_flags + 64 * (size_t)world_ * 2;
    const size_t bytes = ic->off_seq + 256;
    HIPCHK(hipMalloc((void**)&ic->base, bytes));
    ipc = ic;                                 // (from here on release() frees the inbox)
    HIPCHK(hipMemset(ic->base, 0, bytes));
    hipIpcMemHandle_t h; static_assert(sizeof(hipIpcMemHandle_t) <= 64, "vil_comm_ipc_export hands out 64 bytes");
    HIPCHK(hipIpcGetMemHandle(&h, ic->base));
    memset(handle64, 0, 64); memcpy(handle64, &h, sizeof h);
    ic->peer_base[rank_] = ic->base;
    rank = rank_; world = world_;
    return VIL_OK;
}
int Comm::open_ipc(const void* handles) {
    IpcComm* ic = ipc.get(); if (!ic) return VIL_ERR_INVALID_ARGUMENT;
    for (int r = 0; r < ic->world; ++r) {
        if (r == ic->rank) continue;
        hipIpcMemHandle_t h; memcpy(&h, (const char*)handles + 64 * (size_t)r, sizeof h);
        void* p = nullptr;
        if (hipIpcOpenMemHandle(&p, h, hipIpcMemLazyEnablePeerAccess) != hipSuccess) { (void)hipGetLastError(); return VIL_ERR_COMM; }
        ic->peer_base[r] = p;
    }
    ic->ready = true;
    return VIL_OK;
}
int Comm::join_local(Comm** ranks, const int* devices, int n) {
    // k_sum_peers reads the other contexts' buffers directly: contexts on different devices need peer access in both
    // directions (xGMI / PCIe P2P), checked and enabled here; without it the configuration is refused, not faulted at run time
    for (int a = 0; a < n; ++a) for (int b = 0; b < n; ++b) {
        if (devices[a] == devices[b]) continue;
        int can = 0;
        if (hipDeviceCanAccessPeer(&can, devices[a], devices[b]) != hipSuccess || !can) return VIL_ERR_UNSUPPORTED;
        if (hipSetDevice(devices[a]) != hipSuccess) return VIL_ERR_DEVICE;
        const hipError_t e = hipDeviceEnablePeerAccess(devices[b], 0);
        if (e != hipSuccess && e != hipErrorPeerAccessAlreadyEnabled) return VIL_ERR_UNSUPPORTED;
        (void)hipGetLastError();
    }
    auto lc = std::make_shared<LocalComm>();
    if (pthread_barrier_init(&lc->bar, nullptr, (unsigned)n) != 0) return VIL_ERR_COMM;
    lc->n = n;
    for (int r = 0; r < n; ++r) { ranks[r]->release(devices[r]); ranks[r]->local = lc; ranks[r]->rank = r; ranks[r]->world = n; }
    return VIL_OK;
}
