// vilwindow.hip -- the LiDAR frame slabs and the fully resident window of libvilsolve.so (vil_resident.hpp; device layout: vil_window.hpp): slot bookkeeping,
// the per-frame staging DMA, allocation (every buffer a vilhost::Grown: no teardown of its own), and the kernels only this store launches.
#include <algorithm>
#include <cstring>
#include "vil_resident.hpp"
#include "vil_factors.hpp"

struct WinFrameIn {           // one pushed frame, staged in device memory by a single DMA
    int n_obs; const int* track; const double* obs;          // n_obs x VIL_WIN_OBS
    double* store; int T, fslot;
    int ns; const double* samp;                              // [hdr 12 | dt ns | acc 3 ns | gyr 3 ns]
    double* hdr; double* dt; double* acc; double* gyr;       // the IMU slot's arrays
};
// blocks [0, nbo): observations scattered into the store (thread = (observation, component)); the rest: samples into the IMU slot
__global__ __launch_bounds__(256) void k_win_frame_in(WinFrameIn A, int nbo) {
    const int t = threadIdx.x;
    if ((int)blockIdx.x < nbo) {
        const int e = blockIdx.x * 256 + t, o = e >> 3, cidx = e & 7;
        if (o < A.n_obs) A.store[((size_t)A.fslot * A.T + A.track[o]) * VIL_WIN_OBS + cidx] = A.obs[(size_t)o * VIL_WIN_OBS + cidx];
        return;
    }
    const int b = blockIdx.x - nbo, nb = gridDim.x - nbo, ns = A.ns;
    for (int e = b * 256 + t; e < 12 + 7 * ns; e += nb * 256) {
        const double v = A.samp[e];
        if (e < 12) A.hdr[e] = v;
        else if (e < 12 + ns) A.dt[e - 12] = v;
        else if (e < 12 + 4 * ns) A.acc[e - 12 - ns] = v;
        else A.gyr[e - 12 - 4 * ns] = v;
    }
}

// MARGIN_SECOND_NEW (estimator.cpp:1763-1772): the newest interval's samples continue the previous interval's integration
__global__ __launch_bounds__(256) void k_win_append(double* dt, double* acc, double* gyr, int n0, const double* sdt, const double* sacc, const double* sgyr, int n1) {
    for (int e = blockIdx.x * 256 + threadIdx.x; e < 7 * n1; e += gridDim.x * 256) {
        if (e < n1) dt[n0 + e] = sdt[e];
        else if (e < 4 * n1) acc[3 * n0 + e - n1] = sacc[e - n1];
        else gyr[3 * n0 + e - 4 * n1] = sgyr[e - 4 * n1];
    }
}

// sqrt-information of one pre-integration record (imu_factor.h:64: LLT(cov^-1).matrixL()^T), once per record instead of once per upload
__global__ __launch_bounds__(VIL_THREADS) void k_imu_sqrtinfo(const double* rec, double* U, int* status, int skip_empty) {
    if (skip_empty && !(rec[16] > 0.0)) return;          // an interval without samples (the first frame of a window) is never a factor
    imu_sqrtinfo_wg(rec + 62, U, status);
}

// The new prior goes from the marginalisation kernels' work space straight into the resident prior slot: J0 (n x n column-major), r0,
// x0 = the kept blocks of the device state the factors were linearised at (marginalization_factor.cpp:110-139 keeps the very values),
// and the contractions the sweep's prior role works with (J0^T J0, J0^T r0, r0^T r0).  A non-finite entry raises the status word.
struct PriorCommit {
    int n, nblk; const double* J0; const double* r0; const double* x;      // x: device state [pose 7K | sb 9K | ex 7 | td 1 | ...]
    int K; int kind[VIL_WIN_MAXBLK], index[VIL_WIN_MAXBLK];               // kept blocks with their CURRENT frame index (before the shift)
    double* pJ0; double* pr0; double* px0; double* pH; double* pg0; double* pc0; int* status;
};
__global__ __launch_bounds__(256) void k_prior_commit(PriorCommit A) {
    extern __shared__ double sJ[];                       // J0 (n x n column-major, column stride n + 1: conflict-free column walks) | r0
    const int t = threadIdx.x, b = blockIdx.x, nb = gridDim.x, n = A.n, ns = n + 1;
    double* sr = sJ + (size_t)n * ns;
    bool bad = false;
    for (int e = t; e < n * n; e += 256) { const double v = A.J0[e]; if (!(v - v == 0.0)) bad = true; sJ[(e / n) * ns + (e % n)] = v; if (b == 0) A.pJ0[e] = v; }
    for (int e = t; e < n; e += 256) { const double v = A.r0[e]; if (!(v - v == 0.0)) bad = true; sr[e] = v; if (b == 0) A.pr0[e] = v; }
    if (bad) atomicExch(A.status, VIL_ERR_NON_FINITE);
    if (b == 0 && t == 0) {
        int xo = 0;
        for (int q = 0; q < A.nblk; ++q) {
            const int kind = A.kind[q], idx = A.index[q];
            const double* src = kind == VIL_BLK_POSE ? A.x + 7 * idx : (kind == VIL_BLK_SPEEDBIAS ? A.x + 7 * A.K + 9 * idx : (kind == VIL_BLK_EX ? A.x + 16 * A.K : A.x + 16 * A.K + 7));
            const int gs = (kind == VIL_BLK_POSE || kind == VIL_BLK_EX) ? 7 : (kind == VIL_BLK_SPEEDBIAS ? 9 : 1);
            for (int k = 0; k < gs; ++k) A.px0[xo + k] = src[k];
            xo += gs;
        }
    }
    __syncthreads();
    // the contractions out of LDS (column i of J0 at sJ[i * ns ...]): every workgroup staged the whole matrix (39 kB at n = 70), each computes a slice
    for (int e = b * 256 + t; e < n * n + n + 1; e += nb * 256) {
        if (e < n * n) {
            const int i = e / n, k = e % n;
            const double* ci = sJ + (size_t)i * ns; const double* ck = sJ + (size_t)k * ns;
            double s0 = 0, s1 = 0, s2 = 0, s3 = 0;
            int q = 0;
            for (; q + 3 < n; q += 4) { s0 += ci[q] * ck[q]; s1 += ci[q + 1] * ck[q + 1]; s2 += ci[q + 2] * ck[q + 2]; s3 += ci[q + 3] * ck[q + 3]; }
            for (; q < n; ++q) s0 += ci[q] * ck[q];
            A.pH[e] = (s0 + s1) + (s2 + s3);
        } else if (e < n * n + n) {
            const int i = e - n * n;
            const double* ci = sJ + (size_t)i * ns;
            double s0 = 0, s1 = 0;
            for (int q = 0; q < n; ++q) { if (q & 1) s1 += ci[q] * sr[q]; else s0 += ci[q] * sr[q]; }
            A.pg0[i] = s0 + s1;
        } else {
            double s0 = 0;
            for (int q = 0; q < n; ++q) s0 += sr[q] * sr[q];
            A.pc0[0] = s0;
        }
    }
}

__global__ void k_aos2soa(const double* aos, int n, int ncomp, double* dst, size_t stride) {
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f < n) for (int q = 0; q < ncomp; ++q) dst[(size_t)q * stride + f] = aos[(size_t)f * ncomp + q];
}

// ---- the staging pair -------------------------------------------------------------------------------------------------------------
int FrameStage::begin(hipStream_t stream, size_t bytes, size_t grow_to) {
    HIPCHK(sent.wait());
    if (bytes <= d.cap) return VIL_OK;                   // (the twin is allocated last: it is there only when both are)
    HIPCHK(hipStreamSynchronize(stream));                // (a kernel may still be reading the device twin)
    h.release(); d.release();
    HIPCHK(h.reserve(grow_to, grow_to)); HIPCHK(d.reserve(grow_to, grow_to));
    return VIL_OK;
}
int FrameStage::send(hipStream_t stream, size_t bytes) {
    HIPCHK(hipMemcpyAsync(d.p, h.p, bytes, hipMemcpyHostToDevice, stream));
    HIPCHK(sent.record(stream));
    return VIL_OK;
}

// ---- LiDAR frame slabs --------------------------------------------------------------------------------------------------------------
void LidarSlabs::totals(int* n_plane, int* n_edge) const {
    int np = 0, ne = 0;
    for (auto& sl : slabs) { np += sl.np; ne += sl.ne; }
    *n_plane = np; *n_edge = ne;
}
bool LidarSlabs::frame0_has_points(int K) const { return count() == K && slabs[0].np_all + slabs[0].ne_all > 0; }
void LidarSlabs::chunks(bool plane, int K, std::vector<int>& out) const {
    const int ns = count(), cap = plane ? cap_p : cap_e;
    for (int i = 0; i < ns; ++i) {
        const int m = plane ? slabs[i].np : slabs[i].ne;
        for (int s0 = 0; s0 < m; s0 += VIL_THREADS) { out.push_back(slabs[i].slot * cap + s0); out.push_back(std::min(VIL_THREADS, m - s0)); out.push_back(K - ns + i); }
    }
}
void LidarSlabs::tables(DevP& P) const { P.pl_c = d_pl.p; P.pl_stride = nslot * cap_p; P.ed_c = d_ed.p; P.ed_stride = nslot * cap_e; }
void LidarSlabs::reset() {
    slabs.clear(); free_slots.clear();
    for (int q = nslot - 1; q >= 0; --q) free_slots.push_back(q);
}
void LidarSlabs::drop(int i) {
    free_slots.push_back(slabs[i].slot);
    slabs.erase(slabs.begin() + i);
}
int LidarSlabs::push(hipStream_t stream, int rank, int world, int n_plane, const double* plane, int n_edge, const double* edge, bool* tables_moved) {
    const int np_all = n_plane, ne_all = n_edge;
    *tables_moved = false;
    if (world > 1) {       // factor set sharded over ranks: every rank is handed the whole frame and keeps its contiguous slice
        const int pb = (int)((long long)n_plane * rank / world), pe = (int)((long long)n_plane * (rank + 1) / world);
        const int eb = (int)((long long)n_edge * rank / world), ee = (int)((long long)n_edge * (rank + 1) / world);
        plane += (size_t)7 * pb; n_plane = pe - pb; edge += (size_t)9 * eb; n_edge = ee - eb;
    }
    // capacity: points per slab and number of physical slabs only ever grow (the existing slabs are copied once when they do)
    if (n_plane > cap_p || n_edge > cap_e || free_slots.empty()) {
        const int cp2 = std::max(256, std::max(cap_p, ((n_plane + n_plane / 4 + 255) / 256) * 256)), ce2 = std::max(256, std::max(cap_e, ((n_edge + n_edge / 4 + 255) / 256) * 256));
        const int nns = std::max(nslot, count() + 4);
        vilhost::Grown<double> npl, ned;                 // both new tables before either old one goes
        HIPCHK(npl.reserve((size_t)7 * nns * cp2, (size_t)7 * nns * cp2)); HIPCHK(ned.reserve((size_t)9 * nns * ce2, (size_t)9 * nns * ce2));
        HIPCHK(hipStreamSynchronize(stream));
        for (auto& sl : slabs) {
            for (int q = 0; q < 7 && sl.np; ++q) HIPCHK(hipMemcpyAsync(npl.p + ((size_t)q * nns + sl.slot) * cp2, d_pl.p + ((size_t)q * nslot + sl.slot) * cap_p, 8 * (size_t)sl.np, hipMemcpyDeviceToDevice, stream));
            for (int q = 0; q < 9 && sl.ne; ++q) HIPCHK(hipMemcpyAsync(ned.p + ((size_t)q * nns + sl.slot) * ce2, d_ed.p + ((size_t)q * nslot + sl.slot) * cap_e, 8 * (size_t)sl.ne, hipMemcpyDeviceToDevice, stream));
        }
        HIPCHK(hipStreamSynchronize(stream));
        d_pl = std::move(npl); d_ed = std::move(ned);    // (the old tables go with the temporaries, at the end of this block)
        for (int q = nns - 1; q >= nslot; --q) free_slots.push_back(q);
        cap_p = cp2; cap_e = ce2; nslot = nns;
        *tables_moved = true;
    }
    const size_t need = (size_t)7 * n_plane + (size_t)9 * n_edge;
    { const int st = stage.begin(stream, 8 * need, 8 * (need + need / 4 + 1024)); if (st != VIL_OK) return st; }
    const int slot = free_slots.back(); free_slots.pop_back();
    if (need) {
        double* hs = (double*)stage.h.p; const double* ds = (const double*)stage.d.p;
        if (n_plane) memcpy(hs, plane, 8 * (size_t)7 * n_plane);
        if (n_edge) memcpy(hs + (size_t)7 * n_plane, edge, 8 * (size_t)9 * n_edge);
        { const int st = stage.send(stream, 8 * need); if (st != VIL_OK) return st; }
        // point-major rows -> the component-major tables the sweep reads (coalesced, thread = point)
        if (n_plane) hipLaunchKernelGGL(k_aos2soa, dim3((n_plane + 255) / 256), dim3(256), 0, stream, ds, n_plane, 7, d_pl.p + (size_t)slot * cap_p, (size_t)nslot * cap_p);
        if (n_edge) hipLaunchKernelGGL(k_aos2soa, dim3((n_edge + 255) / 256), dim3(256), 0, stream, ds + (size_t)7 * n_plane, n_edge, 9, d_ed.p + (size_t)slot * cap_e, (size_t)nslot * cap_e);
    }
    slabs.push_back({n_plane, n_edge, slot, np_all, ne_all});
    return VIL_OK;
}

// ---- the fully resident window ------------------------------------------------------------------------------------------------------
void Window::release_tables() {
    for (vilhost::Grown<double>* t : {&d_store, &d_samp, &d_hdr, &d_rec, &d_U, &d_prior[0], &d_prior[1]}) t->release();
    is_open = false;
}
int Window::open(hipStream_t stream, const vil_win_cfg* cf) {
    HIPCHK(hipStreamSynchronize(stream));
    const int nf = cf->K + 2;
    if (!is_open || K != cf->K || T != cf->max_tracks || S != cf->max_samples) {
        release_tables();
        int nblk_max;
        K = cf->K; T = cf->max_tracks; S = cf->max_samples; NF = nf;
        vil_prior_capacity(K, &nmax, &nblk_max, &x0max);
        const auto table = [](vilhost::Grown<double>& t, size_t n) { return t.reserve(n, n); };      // (released above: allocates exactly n doubles)
        HIPCHK(table(d_store, (size_t)NF * T * VIL_WIN_OBS));
        HIPCHK(table(d_samp, (size_t)NF * 7 * S)); HIPCHK(table(d_hdr, (size_t)NF * 12));
        HIPCHK(table(d_rec, (size_t)NF * 287)); HIPCHK(table(d_U, (size_t)NF * 225));
        for (int q = 0; q < 2; ++q) HIPCHK(table(d_prior[q], prior_doubles()));
        HIPCHK(d_wstat.reserve(16, 16));                 // (kept across dimensions)
    }
    HIPCHK(hipMemsetAsync(d_store.p, 0, 8 * (size_t)NF * T * VIL_WIN_OBS, stream));
    HIPCHK(hipMemsetAsync(d_rec.p, 0, 8 * (size_t)NF * 287, stream)); HIPCHK(hipMemsetAsync(d_U.p, 0, 8 * (size_t)NF * 225, stream));
    HIPCHK(hipMemsetAsync(d_wstat.p, 0, 64, stream));
    cfg = *cf; is_open = true;
    fslot.clear(); islot.clear(); free_f.clear(); free_i.clear();
    for (int q = NF - 1; q >= 0; --q) { free_f.push_back(q); free_i.push_back(q); }
    ns.assign(NF, 0); sum_dt.assign(NF, 0.0);
    cur = 0; pn = 0; pm = 0; pkind.clear(); pindex.clear(); pcol.clear();
    return VIL_OK;
}
int Window::push_frame(hipStream_t stream, const vil_win_frame* f) {
    const int n = f->n_samples, no = f->n_obs;
    // one staging block, one DMA: [hdr 12 | dt | acc | gyr | observations | track slots]
    const size_t o_samp = 0, o_obs = 8 * (size_t)(12 + 7 * n), o_trk = o_obs + 8 * (size_t)no * VIL_WIN_OBS, total = o_trk + 4 * (size_t)no + 64;
    { const int st = stage.begin(stream, total, 2 * total + 4096); if (st != VIL_OK) return st; }
    double* hs = (double*)(stage.h.p + o_samp);
    memcpy(hs, f->acc0, 24); memcpy(hs + 3, f->gyr0, 24); memcpy(hs + 6, f->lin_ba, 24); memcpy(hs + 9, f->lin_bg, 24);
    double sum = 0.0;
    if (n) { memcpy(hs + 12, f->dt, 8 * (size_t)n); memcpy(hs + 12 + n, f->acc, 24 * (size_t)n); memcpy(hs + 12 + 4 * (size_t)n, f->gyr, 24 * (size_t)n); for (int q = 0; q < n; ++q) sum += f->dt[q]; }
    if (no) { memcpy(stage.h.p + o_obs, f->obs, 8 * (size_t)no * VIL_WIN_OBS); memcpy(stage.h.p + o_trk, f->obs_track, 4 * (size_t)no); }
    { const int st = stage.send(stream, o_trk + 4 * (size_t)no); if (st != VIL_OK) return st; }
    const int fs = free_f.back(), is = free_i.back();
    free_f.pop_back(); free_i.pop_back();
    WinFrameIn A;
    A.n_obs = no; A.track = (const int*)(stage.d.p + o_trk); A.obs = (const double*)(stage.d.p + o_obs); A.store = d_store.p; A.T = T; A.fslot = fs;
    A.ns = n; A.samp = (const double*)(stage.d.p + o_samp); A.hdr = d_hdr.p + 12 * (size_t)is; A.dt = dt(is); A.acc = acc(is); A.gyr = gyr(is);
    const int nbo = (no * VIL_WIN_OBS + 255) / 256;
    hipLaunchKernelGGL(k_win_frame_in, dim3(nbo + 1), dim3(256), 0, stream, A, nbo);
    if (n > 0) {                                         // the interval's record and its sqrt-information, where the solver will read them
        vpre_launch_slot(stream, n, dt(is), acc(is), gyr(is), d_hdr.p + 12 * (size_t)is, cfg.noise, d_rec.p + 287 * (size_t)is);
        hipLaunchKernelGGL(k_imu_sqrtinfo, dim3(1), dim3(VIL_THREADS), 0, stream, d_rec.p + 287 * (size_t)is, d_U.p + 225 * (size_t)is, d_wstat.p, 1);
    }
    fslot.push_back(fs); islot.push_back(is); ns[is] = n; sum_dt[is] = sum;
    return VIL_OK;
}
void Window::unpush_frame() {
    free_f.push_back(fslot.back()); free_i.push_back(islot.back());
    fslot.pop_back(); islot.pop_back();
}
int Window::drop_frame(hipStream_t stream, int flag, int* lidar_slab) {
    const int n = frames();
    if (flag == VIL_MARGIN_OLD) {
        // frame 0 leaves.  Its IMU slot held the interval that ENDED in it -- not a factor of the window; the interval (0, 1) stays with frame 1
        free_f.push_back(fslot[0]); free_i.push_back(islot[0]);
        fslot.erase(fslot.begin()); islot.erase(islot.begin());
        *lidar_slab = 0;
        return VIL_OK;
    }
    // MARGIN_SECOND_NEW (estimator.cpp:1754-1786): frame n-2 leaves; the newest frame takes its place and its samples continue the interval
    // that ended in n-2 (same first measurement, same linearisation point): appended on the device, re-integrated, re-factored
    const int ia = islot[n - 2], ib = islot[n - 1];
    if (ns[ia] + ns[ib] > S) return VIL_ERR_UNSUPPORTED;
    if (ns[ib] > 0) {
        hipLaunchKernelGGL(k_win_append, dim3(1), dim3(256), 0, stream, dt(ia), acc(ia), gyr(ia), ns[ia], dt(ib), acc(ib), gyr(ib), ns[ib]);
        ns[ia] += ns[ib]; sum_dt[ia] += sum_dt[ib];
        vpre_launch_slot(stream, ns[ia], dt(ia), acc(ia), gyr(ia), d_hdr.p + 12 * (size_t)ia, cfg.noise, d_rec.p + 287 * (size_t)ia);
        hipLaunchKernelGGL(k_imu_sqrtinfo, dim3(1), dim3(VIL_THREADS), 0, stream, d_rec.p + 287 * (size_t)ia, d_U.p + 225 * (size_t)ia, d_wstat.p, 1);
    }
    free_f.push_back(fslot[n - 2]); free_i.push_back(ib);
    fslot.erase(fslot.begin() + (n - 2));                // the newest frame's observations and LiDAR points stay where they are
    islot.erase(islot.begin() + (n - 1));                // ... and it now ends the merged interval
    *lidar_slab = n - 2;
    return VIL_OK;
}
void Window::fill(WinSlots& ws) const {
    ws.T = T; ws.store = d_store.p; ws.fslot = fslot.data(); ws.islot = islot.data(); ws.d_rec = d_rec.p; ws.d_U = d_U.p; ws.sum_dt = sum_dt.data();
    ws.pJ0 = pJ0(cur); ws.pr0 = pr0(cur); ws.px0 = px0(cur); ws.pH = pH(cur); ws.pg0 = pg0(cur); ws.pc0 = pc0(cur);
}
void Window::prior_blocks(vil_prior& p) const {
    p.n = pn; p.nblk = (int)pkind.size(); p.blk_kind = pkind.data(); p.blk_index = pindex.data(); p.blk_col = pcol.data();
}
int Window::commit_prior(hipStream_t stream, int K_, bool old_, int n, int m, int nblk, const int* kind, const int* index, const int* col, const double* J0, const double* r0, const double* x) {
    if (n > nmax || nblk > VIL_WIN_MAXBLK) return VIL_ERR_UNSUPPORTED;
    const int dst = 1 - cur;
    PriorCommit pc; memset(&pc, 0, sizeof pc);
    pc.n = n; pc.nblk = col ? 0 : nblk; pc.J0 = J0; pc.r0 = r0; pc.x = x; pc.K = K_;      // nblk = 0: x0 already in place
    for (int b = 0; b < pc.nblk; ++b) { pc.kind[b] = kind[b]; pc.index[b] = index[b]; }
    pc.pJ0 = pJ0(dst); pc.pr0 = pr0(dst); pc.px0 = px0(dst); pc.pH = pH(dst); pc.pg0 = pg0(dst); pc.pc0 = pc0(dst); pc.status = d_wstat.p;
    const size_t pl = 8 * ((size_t)n * (n + 1) + n + 8);
    if (pl > 48 * 1024 && (int)pl > lds_commit) {        // (hipFuncSetAttribute is not free: raised only when it needs more than it was granted before)
        HIPCHK(hipFuncSetAttribute((const void*)k_prior_commit, hipFuncAttributeMaxDynamicSharedMemorySize, (int)pl));
        lds_commit = (int)pl;
    }
    hipLaunchKernelGGL(k_prior_commit, dim3(16), dim3(256), pl, stream, pc);
    cur = dst; pn = n; pm = m;
    pkind.assign(kind, kind + nblk); pindex.clear(); pcol.clear();
    int c0 = 0;
    for (int b = 0; b < nblk; ++b) {
        pindex.push_back(col ? index[b] : blk_shift(kind[b], index[b], old_, K_)); pcol.push_back(col ? col[b] : c0);
        c0 += blk_cols(kind[b]);
    }
    return VIL_OK;
}
int Window::prior_download(hipStream_t stream, vil_prior_out* out, int* h_word) {
    int& wst = *h_word; wst = 0;
    HIPCHK(hipMemcpyAsync(&wst, d_wstat.p, 4, hipMemcpyDeviceToHost, stream));
    out->n = pn; out->nblk = (int)pkind.size(); out->m = pm;
    if (pn > 0) {
        const size_t n = (size_t)pn;
        int xo = 0;
        for (size_t b = 0; b < pkind.size(); ++b) { out->blk_kind[b] = pkind[b]; out->blk_index[b] = pindex[b]; out->blk_col[b] = pcol[b]; xo += blk_doubles(pkind[b]); }
        HIPCHK(hipMemcpyAsync(out->J0, pJ0(cur), 8 * n * n, hipMemcpyDeviceToHost, stream));
        HIPCHK(hipMemcpyAsync(out->r0, pr0(cur), 8 * n, hipMemcpyDeviceToHost, stream));
        HIPCHK(hipMemcpyAsync(out->x0, px0(cur), 8 * (size_t)xo, hipMemcpyDeviceToHost, stream));
        if (out->A) HIPCHK(hipMemcpyAsync(out->A, pH(cur), 8 * n * n, hipMemcpyDeviceToHost, stream));      // J0^T J0
        if (out->b) HIPCHK(hipMemcpyAsync(out->b, pg0(cur), 8 * n, hipMemcpyDeviceToHost, stream));          // J0^T r0
    }
    HIPCHK(hipStreamSynchronize(stream));
    HIPCHK(hipGetLastError());
    return wst;
}
int Window::prior_set(hipStream_t stream, const vil_prior* pr) {
    if (!pr || pr->n <= 0) { pn = 0; pm = 0; pkind.clear(); pindex.clear(); pcol.clear(); return VIL_OK; }
    const size_t n = (size_t)pr->n;
    int xo = 0;
    for (int b = 0; b < pr->nblk; ++b) xo += blk_doubles(pr->blk_kind[b]);
    if (xo > x0max) return VIL_ERR_INVALID_ARGUMENT;
    const int dst = 1 - cur;
    // J0 | r0 | x0 straight into the slot; k_prior_commit then reads J0 | r0 where it writes them
    HIPCHK(hipStreamSynchronize(stream));
    HIPCHK(hipMemcpy(pJ0(dst), pr->J0, 8 * n * n, hipMemcpyHostToDevice)); HIPCHK(hipMemcpy(pr0(dst), pr->r0, 8 * n, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(px0(dst), pr->x0, 8 * (size_t)xo, hipMemcpyHostToDevice));
    const int st = commit_prior(stream, K, false, pr->n, 0, pr->nblk, pr->blk_kind, pr->blk_index, pr->blk_col, pJ0(dst), pr0(dst), nullptr);
    if (st != VIL_OK) return st;
    HIPCHK(hipStreamSynchronize(stream));
    return VIL_OK;
}
