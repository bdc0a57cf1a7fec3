// vil_comm.hpp -- the multi-GPU exchange of libvilsolve.so behind one type (vilcomm.hip); internal, like vil_internal.h.  Three interchangeable transports
// (RCCL bound at run time, in-process, peer buffers between processes), exactly one or none per context.  The solver asks: sharded? sum this buffer? agree on a status?
#pragma once
#include <hip/hip_runtime.h>
#include <algorithm>
#include <memory>
#include <vector>
#include "vil_host.hpp"
#include "vil_internal.h"

// Owned segments of the per-iteration message [camera part | h_ll, b_l, 1/pivot, scale (L each) | e_A (13 L) | e_O (6 F)]: a landmark's entries are
// non-zero on ONE rank, its owner (contiguous landmark / factor ranges, vil_shard_ranges) -- "sum over the ranks" of that part is "take the owner's value"
// (x + 0 + ... + 0 = x: the same bits).  The library's own exchanges therefore move the camera part of every rank but only the OWNED slice of the landmark
// arrays: per peer 103 + 380 / world kB instead of 390 kB at K = 10 / 1000 landmarks (150 kB at world = 8), and the summing kernel reads one inbox for them.
struct OwnSeg { size_t cam; int Lp, n; int lb[9], fb[9]; };      // n = 0: a plain sum of everything (agreements; RCCL beyond eight ranks)
// first landmark whose factor prefix reaches r / world of the total (lms: factor prefix per landmark, L + 1 entries) -- THE sharding rule of the visual factors
static inline int shard_cut(const std::vector<int>& lms, int L, int r, int world) {
    if (r <= 0) return 0;
    if (r >= world) return L;
    const long long target = (long long)lms[L] * r / world;
    return std::min((int)(std::lower_bound(lms.begin(), lms.end(), (int)target) - lms.begin()), L);
}
struct ncclComm; struct LocalComm; struct IpcComm;      // (vilcomm.hip)
struct __attribute__((visibility("hidden"))) Comm {
    int rank = 0, world = 1;
    OwnSeg own = {0, 0, 0, {0}, {0}};      // every rank's landmark / factor range in the per-iteration message (sharded windows): set_owners
    bool slim_emul = false;                // vil_debug_set_slim_emul
    bool sharded() const { return world > 1 && transport() != 0; }      // a world > 1 context without a transport works un-sharded
    bool ready() const { return transport() != -3; }                    // false: vil_comm_ipc_export without vil_comm_ipc_init
    int transport() const;                                              // 0 none, 1 RCCL, 2 in-process, 3 / -3 peer buffers (opened / exported only): vil_comm_info
    bool slim() const { return own.n > 0 && world > 1 && (rccl != nullptr || (slim_emul && local != nullptr)); }      // the packed per-iteration message (SlimLay)
    bool capturable() const { return ipc != nullptr; }                  // the collective may sit in a captured hipGraph: the library's own kernels, counting in device memory
    bool host_synchronised() const { return local != nullptr; }         // the collective synchronises the stream on the host
    // who owns which slice of the landmark arrays of the message (the same arithmetic on every rank); lms: factor prefix per landmark, L + 1 entries
    void set_owners(const std::vector<int>& lms, int L, int K);
    // sum over the ranks, in stream order: recv = sum of every rank's send (recv may be send).  sym = D > 0: the message starts with a symmetric D x D block;
    // owned_slices: the landmark arrays behind it come from their owners (own); span: doubles of one linear-system set
    int sum(hipStream_t stream, const double* send, double* recv, size_t cnt, int sym, bool owned_slices, size_t span);
    // the ranks agree on a status (the worst one): a rank-asymmetric failure -- only rank 0 holds the IMU / prior factors whose set-up can fail --
    // must not leave the other ranks waiting in the first collective of the solve
    int agree(hipStream_t stream, int st);
    void message_bytes(int D, size_t span, int64_t* bytes_per_peer, int64_t* bytes_full_set) const;
    // installing a transport releases whatever the context had first
    static int unique_id(void* id128);
    int use_rccl(int device, const void* id128, int rank, int world);
    int export_ipc(int device, int rank, int world, size_t max_doubles, void* handle64);
    int open_ipc(const void* handles);
    static int join_local(Comm** ranks, const int* devices, int n);
    void release(int device);      // THE teardown: transport, peer handles, inbox, every staging buffer
private:
    int alloc_agree();
    int ipc_sum(hipStream_t stream, const double* send, double* recv, size_t cnt, int sym, const OwnSeg& seg);
    int slim_sum(hipStream_t stream, const double* send, double* recv, int D, size_t span);
    ncclComm* rccl = nullptr;              // RCCL communicator over xGMI (vil_comm_init)
    std::shared_ptr<LocalComm> local;      // in-process communicator (vil_comm_init_local)
    std::shared_ptr<IpcComm> ipc;          // multi-process peer-buffer exchange (vil_comm_ipc_export / vil_comm_ipc_init)
    vilhost::Grown<double> tmp, slim_buf;  // result of an in-place in-process sum; staging of the packed per-iteration message
    vilhost::Grown<double, true> agree_h; vilhost::Grown<double> agree_d;      // agree(): 64 doubles each, pinned / device (RCCL and peer buffers)
};
