// rtmi_batch_coop_launch.hpp — launchers of the cooperative batch kernels (include/rtmi_batch_coop.h), defined in
// rtmi_batch_coop.hip and called by radiance_enqueue, gather_enqueue and sparse_enqueue in rtmi_batch.hip.  Included after
// rtmi_light_launch.hpp and the three batch launch headers (RadianceBatch, GatherBatch, SparseBatch).
#pragma once

// The waves per SIMD a cooperative batch kernel is compiled for, the precedent's: RTMI_LIGHT_COOP_WPS with NEE or ENV,
// RTMI_ROULETTE_COOP_PLAIN_WPS for the plain estimator.  The host sizes the persistent grid with the same number.
constexpr uint32_t rtmi_batch_coop_wps(bool nee, bool env) { return rtmi_roulette_coop_wps(nee, env); }

// The path kernel of each mode over the batch's items on `blocks` persistent wavefronts.  ext: the pool form of
// plan_traversal; lds: the dynamic LDS of a block (WAVES_PER_BLOCK x CoopLds::words() words); nee / env select the
// estimator (both false: the plain one).  Wavefront b of the grid spills to entries [b * P.spill_cap, (b + 1) *
// P.spill_cap) of P.spill: the caller keeps blocks * WAVES_PER_BLOCK within the buffer's wavefronts.
hipError_t rtmi_batch_coop_launch_radiance(bool ext, bool nee, bool env, uint32_t blocks, size_t lds, hipStream_t stream,
                                           const DevScene &sc, const DevParams &P, const RadianceBatch &B, const DevLights &L,
                                           const DevEnv &E);
hipError_t rtmi_batch_coop_launch_gather(bool ext, bool nee, bool env, uint32_t mode, uint32_t blocks, size_t lds, hipStream_t stream,
                                         const DevScene &sc, const DevParams &P, const GatherBatch &B, const DevLights &L,
                                         const DevEnv &E);
hipError_t rtmi_batch_coop_launch_sparse(bool ext, bool nee, bool env, uint32_t blocks, size_t lds, hipStream_t stream,
                                         const DevScene &sc, const DevCamera &cam, const DevParams &P, const SparseBatch &B,
                                         const DevLights &L, const DevEnv &E);
// end of a cooperative batch launch (one thread): the launch's overflow count status[0] joins the sticky word status[2]
// that rtmi_scene_status reports, and goes back to zero
hipError_t rtmi_batch_coop_launch_end(hipStream_t stream, unsigned int *status);
