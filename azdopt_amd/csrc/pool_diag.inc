// pool_diag.inc -- included at the head of pool_step.inc: what the two diagnostic builds measure in the pool step, as hooks that
// fold to nothing in the product build.  pool_eval / pool_search call them by name; no #if sits inside their bodies.
//
//   product   make                                                  per-wave search counters, flushed once at the end of a launch
//   PROFILE   make PROFILE=1 (AZD_PHASE_PROFILE, DIAG_PROFILE)      per-AGENT counters, flushed behind every call (tools/slow_agents.py)
//   PHASES    make VARIANT=phases EXTRA=-DAZD_WAVE_PHASES=1         the product's flush, plus three phases of a wave's cycle summed per
//             (DIAG_WAVE; tools/wave_phases.py)                     wave: none of PROFILE's counter traffic, so the shares are the product's
//
// Counter slots (Arenas::counters, NUM_COUNTERS per agent; include/azdopt_amd.h: AZD_CTR_*) that differ between the builds.  All
// ticks are of the 100 MHz wall clock.  Every other slot holds the same in all three: 0..12, 15 the public search counters, 16..23 the
// phase ticks of rollout_agent (zero in the product, where PH_NOW() is 0), 25..27 and 29 the evaluator service counters.
//
//   slot  product                                 PROFILE                                           PHASES
//   13    evaluator: the layers in SHADER clocks  the same, and on the agent's own block: ticks     as product
//         (pool_eval; any agent's block)          until a selected node's predictions had arrived
//                                                 (select_small)
//   14    --                                      ... until they were reduced (select_small)        add: acquire fence + PendRec + add_actions
//                                                                                                   with the arrived row (diag_wave_add)
//   24    --                                      the row waited for an evaluator                   take: ticket + wait for its slot
//                                                 (diag_row_waited_for_evaluator)                   (diag_wave_take)
//   28    --                                      the agent waited for a wave after its row was     rollout: the whole of rollout_agent, loading
//                                                 stored (diag_agent_waited_for_wave)               the agent and writing it back included
//                                                                                                   (diag_wave_rollout)
//   30    evaluator: ticks of slots + state rows  when the agent's last call was done, absolute     as product
//         in (pool_eval_stage_ticks)              (pool_last_call_done)
//   31    evaluator: ticks of the layers          when the agent was first touched, absolute        as product
//         (pool_eval_stage_ticks)                 (diag_first_touch)
//
// PoolArgs::stamp[agent]: the product and PHASES store there, once per launch, when the agent was through with the launch's calls
// (ticks from the launch's first workgroup: azd_engine_pool_agent_finish); PROFILE keeps there the moment the agent was last handed
// over -- its row posted to an evaluator queue, or the agent put on a ready queue (diag_stamp_handed_over) -- which slots 24 and 28
// are measured from.
// In a wave's LDS block, s.ctr[30] / s.ctr[31] are the wave's busy ticks and the stamp they are counted from, in every build; they
// never reach Arenas::counters.

// how long the row of `agent` waited for an evaluator (slot 24)
__device__ __forceinline__ void diag_row_waited_for_evaluator(const Arenas &a, const PoolArgs &pl, const uint32_t &agent) {
    if constexpr (DIAG_PROFILE) {
        unsigned long long *st = pl.stamp + agent;
        atomicAdd(&a.counters[(size_t)agent * NUM_COUNTERS + 24], (unsigned long long)wall_clock64() - __hip_atomic_load(st, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
    }
}
// first touched in this launch (slot 31, absolute)
__device__ __forceinline__ void diag_first_touch(const Arenas &a, const uint32_t agent) {
    if constexpr (DIAG_PROFILE) a.counters[(size_t)agent * NUM_COUNTERS + 31] = (unsigned long long)wall_clock64();
}
// PROFILE counts per agent and flushes with every call: the wave's search counters start from zero with every agent taken
template <class LDS>
__device__ __forceinline__ void diag_per_agent_counters_reset(LDS &s) {
    if constexpr (DIAG_PROFILE)
        if (LANE < 24) s.ctr[LANE] = 0;
}
template <class LDS>
__device__ __forceinline__ void diag_per_agent_counters_flush(const Arenas &a, LDS &s, const int t) {
    if constexpr (DIAG_PROFILE) flush_counters(a, s, t);
}
// how long agent t waited for a wave after its row was stored (slot 28)
template <class LDS>
__device__ __forceinline__ void diag_agent_waited_for_wave(LDS &s, const PoolArgs &pl, const uint32_t t) {
    if constexpr (DIAG_PROFILE) CTR_ADD(28, (unsigned long long)wall_clock64() - __hip_atomic_load(pl.stamp + t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
}
// Agent t is through with the launch's calls (lane 0).  Product and PHASES: when, in ticks from the launch's first workgroup -- the
// launch lasts as long as its slowest agent's chain, and the bench line says how far behind the median that is
// (azd_engine_pool_agent_finish; one store per agent and launch).  PROFILE: the absolute time, in slot 30.
__device__ __forceinline__ void pool_last_call_done(const Arenas &a, const PoolArgs &pl, PoolCtl *ctl, const uint32_t t) {
    if constexpr (DIAG_PROFILE) a.counters[(size_t)t * NUM_COUNTERS + 30] = (unsigned long long)wall_clock64();
    else pl.stamp[t] = (unsigned long long)wall_clock64() - __hip_atomic_load(&ctl->t_first, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// the three phases of a searcher wave's cycle, from a WAVE_NOW() stamp taken where the phase began (slots 24, 14, 28)
template <class LDS>
__device__ __forceinline__ void diag_wave_take(LDS &s, const unsigned long long since) {
    WAVE_CTR_ADD(24, WAVE_NOW() - since);
}
template <class LDS>
__device__ __forceinline__ void diag_wave_add(LDS &s, const unsigned long long since) {
    WAVE_CTR_ADD(14, WAVE_NOW() - since);
}
template <class LDS>
__device__ __forceinline__ void diag_wave_rollout(LDS &s, const unsigned long long since) {
    WAVE_CTR_ADD(28, WAVE_NOW() - since);
}
// an evaluator workgroup's split of its batch ticks (slots 30 / 31; PROFILE keeps the agents' first / last stamps there)
__device__ __forceinline__ void pool_eval_stage_ticks(unsigned long long *ctr, const unsigned long long t_stage, const unsigned long long t_layers) {
    if constexpr (!DIAG_PROFILE) {
        atomicAdd(&ctr[30], t_stage);  // ... of which: slots + state-vector rows in
        atomicAdd(&ctr[31], t_layers); // ... of which: the layers
    }
}
// The end of a searcher wave's launch: its counters go to one agent's block (the host sums -- or, for the three maxima, maximises --
// the blocks over the agents, so which block takes them does not matter).
// Product: the search counters of everything this wave has run, once (round 4): a read-modify-write of the agent's block behind every
// call was a dependent round trip (load, then store, then the drain that waits for both) at the end of each call, on the wave's time.
// PHASES: the same, and the take / rollout phases (add is slot 14: below 24).  PROFILE: the calls have flushed per agent
// (diag_per_agent_counters_flush); what is left is slot 28, added behind the last flush of an agent that came back with a row.
// (A macro, not a function like the hooks above: as a function it cost PROFILE's k_pool / k_pool_search 40 bytes of other code.)
#define POOL_SEARCH_FLUSH(a, s, B)                                                                                                                \
    do {                                                                                                                                          \
        if constexpr (DIAG_PROFILE) {                                                                                                             \
            if (LANE == 0 && s.ctr[28])                                                                                                           \
                atomicAdd(&a.counters[(size_t)((blockIdx.x * PERSIST_WAVES + (threadIdx.x >> 6)) % B) * NUM_COUNTERS + 28], s.ctr[28]);           \
        } else {                                                                                                                                  \
            WAVE_SYNC();                                                                                                                          \
            if constexpr (DIAG_WAVE)                                                                                                              \
                if ((LANE == 24 || LANE == 28) && s.ctr[LANE])                                                                                    \
                    atomicAdd(&a.counters[(size_t)((blockIdx.x * PERSIST_WAVES + (threadIdx.x >> 6)) % B) * NUM_COUNTERS + LANE], s.ctr[LANE]);   \
            if (LANE < 24) {                                                                                                                      \
                const unsigned long long v = s.ctr[LANE];                                                                                         \
                unsigned long long *ctr = a.counters + (size_t)((blockIdx.x * PERSIST_WAVES + (threadIdx.x >> 6)) % B) * NUM_COUNTERS;            \
                if (LANE == 10 || LANE == 11 || LANE == 21) atomicMax(&ctr[LANE], v);                                                             \
                else if (v) atomicAdd(&ctr[LANE], v);                                                                                             \
            }                                                                                                                                     \
        }                                                                                                                                         \
    } while (0)
