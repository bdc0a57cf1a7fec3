/* vilvgicp_voxel.h -- the target voxel map of include/vilvgicp.h built on the device, and a resident source promoted to the next
 * target.  Included by vilvgicp.h: a caller never names this file.  Account of the contract, the kernels and the measurements:
 * docs/voxelmap.md.
 *
 * The map is GaussianVoxelMap::create_voxelmap (gicp/fast_vgicp_voxel.hpp:107-159, ADDITIVE voxels): voxels numbered in the order of
 * their first point, per voxel the sequential double sums of the points and of their covariances in ascending point index, divided by
 * the count.  Both builders give the same bits in every field; they differ in where the work is done. */
#ifndef VILVGICP_VOXEL_H
#define VILVGICP_VOXEL_H
#include "vilvgicp.h"
#ifdef __cplusplus
extern "C" {
#endif

enum { VGICP_BUILD_HOST = 0, VGICP_BUILD_DEVICE = 1 };
/* default HOST: covariances copied down, the map summed on the host, six buffers uploaded.  DEVICE: the points (and the covariances,
 * when given) are uploaded, everything else happens on the device and one host wait brings back the voxel count and the non-finite
 * flag.  Takes effect at the next vgicp_set_target, also inside vloop_verify (villoop.h), which is handed this context. */
int vgicp_set_voxel_builder(vgicp_ctx* ctx, int32_t builder);
/* The resident source (points and covariances, as vgicp_set_source left them) becomes the target at `resolution`, on the device
 * whatever the builder; the source stays resident.  The reference estimates the covariances of scan j twice, as source and as the
 * next pair's target: the same function of the same points, so this reuse is exact.  VIL_ERR_INVALID_ARGUMENT without a source;
 * VIL_ERR_NON_FINITE for a non-finite coordinate, and the previous target then stays usable and unchanged (as with the device builder
 * in vgicp_set_target). */
int vgicp_promote_source(vgicp_ctx* ctx, double resolution);
/* Test / logging hook: the target map in voxel order, of either builder.  Arrays may be NULL; count is always set;
 * VIL_ERR_INVALID_ARGUMENT when capacity < count (nothing is written then).  keys: the packed voxel coordinates, 21 bits per axis. */
typedef struct vgicp_voxels {
    int32_t capacity, count;
    int64_t* keys;
    int32_t* num;
    double* mean3;
    double* cov9;
    double* wsq;
} vgicp_voxels;
int vgicp_read_voxels(vgicp_ctx* ctx, vgicp_voxels* out);
/* HIP events around the device builder's kernels, in launch order: k_vox_clear, k_vox_insert, k_vox_offsets, k_vox_fill, k_vox_scan,
 * k_vox_rank, k_vox_sum.  vgicp_build_profile_read fills VGICP_BUILD_KERNELS launch counts and total milliseconds, and resets both. */
#define VGICP_BUILD_KERNELS 7
int vgicp_build_profile_enable(vgicp_ctx* ctx, int32_t enable);
int vgicp_build_profile_read(vgicp_ctx* ctx, int64_t* launches, double* total_ms);

#ifdef __cplusplus
}
#endif
#endif
