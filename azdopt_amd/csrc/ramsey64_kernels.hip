// ramsey64_kernels.hip -- the 64-bit tier of the Ramsey space (AZD_ENGINE_RAMSEY_U64: N <= 64 over uint64_t neighbourhood rows,
// E*C <= 2304, keys of 36 words): tree_core.inc instantiated with RamseyU64Space (space_ramsey.inc) in a translation unit of its
// own, so that its kernels' register allocation and build time stay apart from the 32-bit tiers'.  Launch-per-phase kernels and the
// device root policy; ramsey_kernels.hip forwards to these launchers for engines with ramsey_u64(a).
// Built with -ffp-contract=off like the other search units.
#include <hip/hip_runtime.h>

#include "engine_types.h"

namespace azd {

#include "tree_core.inc"
#include "space_ramsey.inc"
#include "persistent_step.inc"
#include "root_policy.inc"

using SP64 = RamseyU64Space;

void ramsey64_launch_modify_roots(const Arenas &a, uint64_t seed, uint64_t epoch, uint64_t first_agent, int kmin, int kmax,
                                  uint8_t *d_colors, uint64_t *d_perm, void *stream) {
    k_modify_roots<SP64><<<dim3(a.B), dim3(64), SP64::dyn_bytes(a), (hipStream_t)stream>>>(a, seed, epoch, first_agent, kmin, kmax, d_colors, d_perm, d_perm);
}
void ramsey64_launch_init_roots(const Arenas &a, const uint8_t *d_colors, const uint64_t *d_permitted, void *stream) {
    k_init_roots<SP64><<<dim3(a.B), dim3(64), SP64::dyn_bytes(a), (hipStream_t)stream>>>(a, d_colors, d_permitted);
}
void ramsey64_launch_add_actions(const Arenas &a, int root_mode, void *stream) {
    k_add_actions<SP64><<<dim3(a.tn ? a.tn : a.B), dim3(64), SP64::dyn_bytes(a), (hipStream_t)stream>>>(a, root_mode);
}
void ramsey64_launch_rollout(const Arenas &a, const TolTable &tol, void *stream) {
    k_rollout<SP64><<<dim3(a.tn ? a.tn : a.B), dim3(64), SP64::dyn_bytes(a), (hipStream_t)stream>>>(a, tol);
}
void ramsey64_launch_argmin_one(const Arenas &a, int agent, uint32_t node, void *stream) {
    k_argmin_one<SP64><<<dim3(1), dim3(64), SP64::dyn_bytes(a), (hipStream_t)stream>>>(a, agent, node);
}
void ramsey64_launch_argmin_log(const Arenas &a, int n_calls, unsigned long long *log_key, void *stream) {
    k_argmin_log1<SP64><<<dim3(1), dim3(64), SP64::dyn_bytes(a), (hipStream_t)stream>>>(a, n_calls, log_key, nullptr);
}
void ramsey64_launch_argmin(const Arenas &a, int init_mode, void *stream) {
    k_argmin<SP64><<<dim3(1), dim3(1024), SP64::dyn_bytes(a), (hipStream_t)stream>>>(a, init_mode);
}
void ramsey64_launch_observe(const Arenas &a, uint32_t n_obs_tol, void *stream) {
    k_observe<SP64><<<dim3(a.B), dim3(64), SP64::dyn_bytes(a), (hipStream_t)stream>>>(a, n_obs_tol);
}

} // namespace azd
