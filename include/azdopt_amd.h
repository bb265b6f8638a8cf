/*
 * azdopt_amd.h -- C ABI of the MI355X-native self-play hot path of ariasanovsky/azdopt.
 *
 * The reference has no FFI layer; its seams are Rust traits.  Each entry point
 * below replaces one trait method / pub fn (cited as file:line relative to the
 * reference root) with the same argument meaning, ownership and layout:
 *
 *   evaluator seam   trait NablaModel              az-discrete-opt/src/nabla/model/mod.rs:4-8
 *                    ActionModel::{new,...}        az-discrete-opt/src/nabla/model/dfdx.rs:36-131
 *   engine seam      NablaOptimizer pub methods    az-discrete-opt/src/nabla/optimizer/mod.rs:30-36,39,121,249,284,361
 *   space seam       NablaStateActionSpace         az-discrete-opt/src/nabla/space/mod.rs:5-39
 *                    (device-resident spaces are built in and selected by id;
 *                     the trait stays the host-side description)
 *
 * Conventions: plain pointers and sizes, no torch types.  Host slices are lent
 * for the duration of the call (as the Rust `&[f32]` / `&mut [f32]` are) and are
 * never retained.  All matrices are row-major, agent-major.  Every function
 * returns an azd_status (0 = OK); nothing aborts the process (the reference
 * panics with panic='abort', graph-state/Cargo.toml:59,62).
 *
 * The library has NO CPU fallback: every compute entry point runs HIP kernels
 * on a gfx950 device and fails with AZD_ERR_NO_DEVICE when none is present.
 */
#ifndef AZDOPT_AMD_H
#define AZDOPT_AMD_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef enum azd_status {
    AZD_OK = 0,
    AZD_ERR_INVALID_ARGUMENT = 1,
    AZD_ERR_NO_DEVICE = 2,
    AZD_ERR_HIP = 3,
    AZD_ERR_CAPACITY = 4,      /* a tree arena (nodes / arcs / predictions / frontier) overflowed */
    AZD_ERR_UNREACHABLE = 5,   /* the reference's unreachable!() at tree/mod.rs:227 */
    AZD_ERR_NO_EVALUATOR = 6,  /* engine created without an evaluator: use the *_begin/_end pair */
    AZD_ERR_OUT_OF_MEMORY = 7,
    AZD_ERR_UNSUPPORTED = 8
} azd_status;

const char *azd_status_string(int status);
/* text of the last HIP error seen by the calling thread ("" if none) */
const char *azd_last_error(void);
int azd_version(void);
/* number of visible gfx950 devices (0 on a box without a GPU; never fails) */
int azd_device_count(void);

/* ------------------------------------------------------------------------- */
/* Space seam: c21 = ROTModifyParentsOnce<N, Conjecture2Dot1Cost>            */
/*   graph-state/src/rooted_tree/space.rs:14-125                             */
/* ------------------------------------------------------------------------- */
#define AZD_SPACE_C21 1
#define AZD_C21_MAX_N 24
int azd_c21_state_dim(int n);  /* (N-1)(N-2)-2     space.rs:46 */
int azd_c21_action_dim(int n); /* (N-1)(N-2)/2-1   space.rs:48 */
int azd_c21_key_words(int n);  /* u64 words of an ActionSet bit mask */

/* Host-side `init_states` closure of the driver (04-c21-tree.rs:108-112;
 * rooted_tree/mod.rs:14-20; modify_parent_once.rs:14-25) with a seeded,
 * counter-based generator instead of thread_rng (spec: DESIGN.md).
 * Packed root format used everywhere below:
 *   parents   [count][n]  u8   parents[v] < v, parents[0]=parents[1]=parents[n-1]=0
 *   permitted [count][KW] u64  bit a set <=> action id a is permitted */
int azd_c21_generate_roots(uint64_t seed, uint64_t epoch, uint64_t first_agent, int count, int n,
                           int kmin, int kmax, uint8_t *parents, uint64_t *permitted);

/* ------------------------------------------------------------------------- */
/* Space seam: Ramsey = RamseySpaceNoEdgeRecolor<B32, N, E, C>               */
/*   graph-state/src/ramsey_counts/space.rs:10-176 (drivers 01-r333.rs,      */
/*   02-r44.rs): E = N(N-1)/2 edges in colex order (simple_graph/edge.rs),   */
/*   action id = edge + new_colour * E.  Built for E <= 256, 2..4 colours,   */
/*   clique sizes 2..5, E*C <= 384 (r333: N=16, r44: N=17).  A WIDE engine  */
/*   (azd_engine_config::max_slots > 0) takes N <= 32, E*C <= 1024 and up to */
/*   max_slots permitted edges per root (r45: N=24, 276 edges).  With       */
/*   AZD_ENGINE_RAMSEY_U64 beside max_slots > 0 the engine runs the 64-BIT   */
/*   tier: N <= 64 over 64-bit neighbourhood words, E*C <= 2304, a node of   */
/*   up to 512 actions (r3333: N=34, four colours, 561 edges).  With         */
/*   AZD_ENGINE_RAMSEY_BIG_CLIQUES beside that flag: clique sizes 2..8       */
/*   (R(4,6): N=35), within the reference's i32 bound (see the flag).        */
/* ------------------------------------------------------------------------- */
#define AZD_SPACE_RAMSEY 2
/* (narrow tier: E <= 256 alone would allow N = 23, but E*C <= 384 with C >= 2 bounds it at N = 20 -- E = 190, E*C = 380; with
 * three colours at N = 16, with four at N = 14.  No narrow engine of N = 21..23 is accepted; the constant stays as it is: ABI) */
#define AZD_RAMSEY_MAX_N 23
#define AZD_RAMSEY_WIDE_MAX_N 32
#define AZD_RAMSEY_U64_MAX_N 64
#define AZD_RAMSEY_U64_NODE_ACTIONS 512 /* 64-bit tier: max_slots * (C - 1) may not exceed it */
#define AZD_RAMSEY_BIG_CLIQUE_MAX 8     /* 64-bit tier with AZD_ENGINE_RAMSEY_BIG_CLIQUES: the largest forbidden clique */
int azd_ramsey_state_dim(int n, int n_colors);  /* E(2C+1)  space.rs:40 */
int azd_ramsey_action_dim(int n, int n_colors); /* EC       space.rs:42 */
int azd_ramsey_key_words(int n, int n_colors);
/* Host-side `init_state` closure of the drivers (01-r333.rs:84-90: ColoredCompleteBitsetGraph::
 * generate with uniform colour weights + RamseyCountsNoRecolor::generate), seeded.
 * Packed root format of this space, passed through the same `parents` / `permitted`
 * arguments of the engine calls below:
 *   colors    [count][E]  u8   colour of the edge at each colex position
 *   permitted [count][KW] u64  bit e set <=> edge position e may still be recoloured */
int azd_ramsey_generate_roots(uint64_t seed, uint64_t epoch, uint64_t first_agent, int count, int n,
                              int n_colors, int kmin, int kmax, uint8_t *colors, uint64_t *permitted);
/* The same with colour weights (05-r45.rs:84-90: WeightedIndex([P_RED, P_BLUE])): color_weights[n_colors], finite and
 * positive; NULL is azd_ramsey_generate_roots.  k and the shuffle take the same draws; only the colour of an edge differs.
 * Integer-only once the thresholds exist, so host, device and any restatement agree bit for bit:
 *   cum_c = cum_{c-1} + w_c in f64, in colour order;  W = cum_{C-1};
 *   T_c = min(2^32, ceil((cum_c / W) * 4294967296.0)) for c < C - 1, a 64-bit integer;
 *   colour of edge e = #{ c < C - 1 : (r >> 32) >= T_c } with r the edge's draw 1024 + e.
 * Equal weights give the uniform draw for C = 2, 3, 4. */
int azd_ramsey_generate_roots_weighted(uint64_t seed, uint64_t epoch, uint64_t first_agent, int count, int n,
                                       int n_colors, int kmin, int kmax, const double *color_weights, uint8_t *colors,
                                       uint64_t *permitted);

/* ------------------------------------------------------------------------- */
/* Space seam: dense graphs (BUILD-DEFINED: the reference has no live         */
/*   NablaStateActionSpace over general graphs, examples/05-ah.rs is a stub)  */
/*   built from ConnectedBitsetGraph (connected_bitset_graph/mod.rs:45-71,    */
/*   139-158, 226-338), AddOrDeleteEdge (bitset_graph/space/action.rs:4-27)   */
/*   and the STATE = E + ACTION + 1 hint (05-ah.rs:39-40); definition in      */
/*   oracle/dense_graph.inc.  BASELINE.json configs[4]: N = 50.               */
/*   The objective is a choice: Conjecture2Dot1Cost (lambda_1 + matching      */
/*   number; mod.rs:319-338), the default, or -- with the engine flag         */
/*   AZD_ENGINE_DENSE_AH, N <= AZD_DENSE_AH_MAX_N = 32 -- the Aouchiche-      */
/*   Hansen cost that 05-ah.rs searches with (ah_cost, mod.rs:156-198;        */
/*   azd_dense_ah_cost below), or up to N = 64 with                           */
/*   AZD_ENGINE_DENSE_AH_WIDE beside it.  States, actions, vectors and roots  */
/*   are the same for all of them.  A third choice, AZD_ENGINE_DENSE_INV      */
/*   (N <= 32), is a weighted combination of ten graph invariants whose      */
/*   weights are given at run time (azd_dense_inv_cost below).                */
/* ------------------------------------------------------------------------- */
#define AZD_SPACE_DENSE 3
#define AZD_DENSE_MAX_N 64
#define AZD_DENSE_MAX_SLOTS 1024 /* modifiable edge slots of a root = legal actions a node can hold (azd_engine_config::max_slots) */
int azd_dense_state_dim(int n);  /* 3E + 1 */
int azd_dense_action_dim(int n); /* 2E: Add(e) = e, Delete(e) = E + e */
int azd_dense_key_words(int n);  /* u64 words of an action-id set */
/* Seeded `init_states`: a connected G(n, p) (redrawn until connected, as ConnectedBitsetGraph::generate does) and
 * k in [kmin, kmax] modifiable edge slots.  Packed root format of this space:
 *   adj   [count][n]  u64  neighbourhood bitsets (passed as the `parents` bytes of the engine calls: 8 n bytes per root)
 *   slots [count][KW] u64  bit e set <=> the edge slot at colex position e may be modified (once) */
int azd_dense_generate_roots(uint64_t seed, uint64_t epoch, uint64_t first_agent, int count, int n, int kmin, int kmax,
                             double p, uint64_t *adj, uint64_t *slots);

/* ------------------------------------------------------------------------- */
/* Evaluator seam (NablaModel)                                               */
/* ------------------------------------------------------------------------- */
typedef struct azd_evaluator azd_evaluator;

typedef struct azd_adam_config { /* dfdx AdamConfig as set at 04-c21-tree.rs:87-92 */
    float lr;
    float beta1;
    float beta2;
    float eps;
    float l2; /* WeightDecay::L2 */
} azd_adam_config;

#define AZD_ACT_NONE 0
#define AZD_ACT_RELU 1
#define AZD_ACT_SIGMOID 2

/* ActionModel::new (model/dfdx.rs:36-53): an MLP state_dim -> hidden[0] -> ... -> action_dim,
 * ReLU between layers, `final_act` on the head (04-c21-tree.rs:46-52), fp32, Adam. */
int azd_evaluator_create_mlp(azd_evaluator **out, int device, int max_batch, int state_dim,
                             int action_dim, const int *hidden, int n_hidden, int final_act,
                             const azd_adam_config *adam, uint64_t seed);
/* TrivialModel (model/mod.rs:10-23): leaves predictions untouched, loss 0. */
int azd_evaluator_create_trivial(azd_evaluator **out, int device, int state_dim, int action_dim);
/* Fixed prediction stream h(agent, call, a): the parity harness'
 * stand-in for a model, so MLP rounding cannot perturb tree topology. */
int azd_evaluator_create_hash_stream(azd_evaluator **out, int device, int state_dim, int action_dim,
                                     uint64_t seed, uint64_t first_agent);
int azd_evaluator_destroy(azd_evaluator *ev);

/* NablaModel::write_predictions (model/mod.rs:5; dfdx.rs:69-84).
 * states: batch*state_dim, predictions: batch*action_dim, host memory. */
int azd_evaluator_write_predictions(azd_evaluator *ev, int batch, const float *states,
                                    float *predictions);
/* NablaModel::update_model (model/mod.rs:6-7; dfdx.rs:86-131): w /= sum(w);
 * L = sum w (pred - obs)^2; backward; Adam.  Returns L in *loss. */
int azd_evaluator_update_model(azd_evaluator *ev, int batch, const float *states,
                               const float *observations, const float *action_weights, float *loss);
/* Same two calls on DEVICE pointers (what the engine uses internally and what a
 * multi-GPU host calls after its all-gather).  `stream` is a hipStream_t or NULL. */
int azd_evaluator_write_predictions_dev(azd_evaluator *ev, int batch, const float *d_states,
                                        float *d_predictions, void *stream);
int azd_evaluator_update_model_dev(azd_evaluator *ev, int batch, const float *d_states,
                                   const float *d_observations, const float *d_action_weights,
                                   float *loss, void *stream);
/* flat parameter vector: per layer W[out][in] then b[out] (dfdx Linear layout) */
/* Weight storage of the MLP evaluator for INFERENCE (write_predictions and the in-kernel evaluator):
 * AZD_STORAGE_BF16 = weights and layer inputs rounded to bf16 (RNE), products exact, f32 accumulate
 * (v_mfma_f32_16x16x16_bf16), biases and outputs f32; the optimiser keeps f32 master weights and the bf16
 * copy is refreshed after every step (BASELINE config C: "bf16 storage / fp32 accumulate").  Default f32. */
#define AZD_STORAGE_F32 0
#define AZD_STORAGE_BF16 1
int azd_evaluator_set_weight_storage(azd_evaluator *ev, int dtype);
int64_t azd_evaluator_num_params(azd_evaluator *ev);
int azd_evaluator_get_params(azd_evaluator *ev, float *out);
int azd_evaluator_set_params(azd_evaluator *ev, const float *in);
/* number of evaluator invocations so far (the `call` index of the hash stream) */
uint64_t azd_evaluator_calls(azd_evaluator *ev);

/* ------------------------------------------------------------------------- */
/* Engine seam (NablaOptimizer<Space, M, ActionSet>)                         */
/* ------------------------------------------------------------------------- */
typedef struct azd_engine azd_engine;

/* Upper limits of the per-tree arenas (what the packed prediction record holds; the reference's petgraph indices are u32 and
 * have none): azd_engine_create refuses a configuration beyond them with AZD_ERR_INVALID_ARGUMENT and an azd_last_error()
 * that names the argument. */
#define AZD_MAX_NODE_CAPACITY 65536
#define AZD_MAX_ARC_CAPACITY 65535
#define AZD_MAX_PREDICTION_CAPACITY (1 << 20)

typedef struct azd_engine_config {
    int space_id;      /* AZD_SPACE_C21 or AZD_SPACE_RAMSEY */
    int n;             /* vertices N (c21: 4..AZD_C21_MAX_N; Ramsey: 3..AZD_RAMSEY_MAX_N, wide: ..AZD_RAMSEY_WIDE_MAX_N, 64-bit tier: ..AZD_RAMSEY_U64_MAX_N) */
    int batch;         /* BATCH: agents (trees) owned by this engine / GPU */
    int device;        /* HIP device ordinal */
    /* per-tree arena capacities; 0 = default sized for 800 calls per epoch (4096 / 8192 / 32768).  Upper limits, from what a
     * prediction record packs (node ids 16 bits, arc ids 16, a node's first prediction 20): 65536 nodes, 65535 arcs, 1048576
     * predictions per tree; ACTION_DIM <= 4096, <= 2047 actions per node.  Beyond them azd_engine_create returns
     * AZD_ERR_INVALID_ARGUMENT; an arena that fills during a run stops its agent and surfaces as AZD_ERR_CAPACITY. */
    int node_capacity;
    int arc_capacity;
    int prediction_capacity;
    uint64_t first_agent; /* global id of agent 0 (multi-GPU sharding) */
    uint32_t flags;       /* AZD_ENGINE_* */
    /* AZD_SPACE_RAMSEY only (RamseySpaceNoEdgeRecolor::new(sizes, weights), space.rs:17-24) */
    int n_colors;         /* C */
    int clique_sizes[4];  /* SIZES: forbidden clique size per colour */
    float color_weights[4];
    /* path encoding P of NablaOptimizer<Space, M, P> (az-discrete-opt/src/path/, licences in
     * space/axioms.rs:12-19); both built spaces are ActionsNeverRepeat + ActionOrderIndependent */
    int path_kind;        /* AZD_PATH_* */
    /* Layered<L, Space> history wrapper (az-discrete-opt/src/space/layered.rs; nabla/space/mod.rs:41-111):
     * 0 or 1 = plain space; L = 2..8: STATE_DIM becomes L * inner STATE_DIM and a state vector carries the
     * last L states of the agent's path, oldest first; chunks of states the ring does not hold yet keep
     * their earlier contents, as in the reference.  A root installed by par_new / par_reset_trees is a ring
     * of one (Layers::new). */
    int layers;
    /* AZD_SPACE_DENSE only: the most modifiable edge slots a root may bring (= legal actions a node can hold); 0 = 128.  The
     * engine keeps transposition keys over the ranks of a root's slots in 2, 4, 10 or 16 words: up to 128, 256, 640 or 1024
     * slots (E / 2 = 612 at N = 50).  dense_p: edge probability of the fresh roots the device root policy draws (the `p` of
     * azd_dense_generate_roots; 0 = 0.2).
     * AZD_SPACE_RAMSEY: 0 = today's limits (E <= 256, E*C <= 384, at most 128 / (C - 1) permitted edges per root).  1..E makes the
     * engine WIDE: 3 <= n <= AZD_RAMSEY_WIDE_MAX_N, E*C <= 1024, a root may bring up to max_slots permitted edges (a node then
     * holds up to max_slots * (C - 1) legal actions); ActionSet paths only, no Layered wrapper.  Its argmin is read with
     * azd_engine_ramsey_wide_argmin_data.  With AZD_ENGINE_RAMSEY_U64 in `flags`: the 64-bit tier's limits (see the flag). */
    int max_slots;
    float dense_p;
} azd_engine_config;
/* ActionSet (path/set.rs): key = set of actions taken; equal sets share a node (transpositions).
 * ActionMultiset (path/multiset.rs) coincides with it on ActionsNeverRepeat spaces: every count is 1,
 * so identity, Ord and len are the set's. */
#define AZD_PATH_SET 0
/* ActionSequence (path/sequence.rs) and OrderedActionSet (path/ord_set.rs, also a Vec that
 * push_unchecked appends to): key = actions in the order taken; a path only ever meets itself, so
 * the search graph is a tree, and BTreeMap order = lexicographic order of the sequences. */
#define AZD_PATH_SEQUENCE 1

/* run every phase of a call as its own kernel launch instead of the CU-resident persistent step
 * (the two forms produce identical trees; the persistent step is the fast one) */
#define AZD_ENGINE_NO_PERSISTENT_STEP 1u
/* The CU-resident step comes in three forms with identical results.  With none of the three flags below the
 * engine takes the pool step for populations of 256 agents and more and the asynchronous step below that, and
 * falls back by itself (pool -> asynchronous -> lock-step -> one launch per phase) when a form cannot take the
 * model; azd_engine_step_form says which form ran and why.
 * AZD_ENGINE_ASYNC_STEP: k_async -- one workgroup = 16 agents on 16 wavefronts, the agents of a workgroup drift
 * apart, an agent waiting for its prediction row serves MFMA tile tasks of the workgroup's evaluator (hidden layer
 * widths in multiples of 16, input width in multiples of 4).
 * AZD_ENGINE_BARRIER_STEP: k_persist -- the same residency in lock-step (a workgroup barrier around the evaluator
 * on every call), 12 % slower at 4096 agents (profiles/README.md). */
#define AZD_ENGINE_ASYNC_STEP 2u
#define AZD_ENGINE_BARRIER_STEP 4u
/* Third CU-resident form, identical results again (k_pool): agents are not bound to wavefronts -- searcher
 * workgroups pull ready agents from per-XCD queues and never wait for a prediction row, evaluator workgroups on
 * CUs of their own pull batches of up to 16 posted rows (full MFMA row tiles, an undisturbed weight stream).
 * Populations larger than the resident waves share them instead of running as serial rounds of workgroups. */
#define AZD_ENGINE_POOL_STEP 8u
/* AZD_SPACE_RAMSEY with max_slots > 0 only: the 64-bit tier.  3 <= n <= AZD_RAMSEY_U64_MAX_N (neighbourhoods are 64-bit words, the
 * reference's B64), E*C <= 2304 (keys of 36 words: N = 34 at four colours, 39 at three, 48 at two), 2..4 colours, clique sizes
 * 2..5 (2..AZD_RAMSEY_BIG_CLIQUE_MAX with AZD_ENGINE_RAMSEY_BIG_CLIQUES beside this flag), 1 <= max_slots <= E and
 * max_slots * (C - 1) <= AZD_RAMSEY_U64_NODE_ACTIONS; ActionSet paths only, no Layered wrapper.
 * Never chosen from the sizes: without the flag every limit, kernel and error text is the 32-bit tiers'.  Shapes a 32-bit wide
 * engine takes are accepted too and give the same trees.  Runs the launch-per-phase step form (the other CU-resident forms fall
 * back, azd_engine_step_form gives the reason) or, with AZD_ENGINE_EXT_POOL_STEP beside it and a bf16 model, the searcher-only pool
 * step (r3333 at 512 agents 1.53 M expansions/s against 1.00 M, r45 at 256 agents 0.97 M against 0.29 M); its argmin is read with
 * azd_engine_ramsey_argmin_any. */
#define AZD_ENGINE_RAMSEY_U64 16u
/* The dense-graph space with the Aouchiche-Hansen cost (azd_dense_ah_cost below; the objective of the reference's
 * examples/05-ah.rs) where a dense engine minimises lambda_1 + matching number by default.  Valid only with AZD_SPACE_DENSE,
 * never inferred from sizes; without it every limit, kernel and error text is the default's.  Limits, refused by
 * azd_engine_create with AZD_ERR_INVALID_ARGUMENT and an azd_last_error() naming the argument: 4 <= n <= AZD_DENSE_AH_MAX_N,
 * layers <= 1, max_slots <= E, ActionSet paths.  State vector, actions, keys, roots and root policy are the dense space's.
 * Such an engine keeps (proximity, eigenvalue, diameter, k) per agent where the default keeps (lambda_1, matching size), and no
 * per-node matching arena; read them with azd_engine_dense_ah_agent_cost and azd_engine_dense_ah_argmin_data
 * (azd_engine_dense_argmin_data, and azd_engine_agent_state's lambda_1 / matching_size, are AZD_ERR_UNSUPPORTED on it). */
#define AZD_ENGINE_DENSE_AH 32u
/* Beside AZD_ENGINE_DENSE_AH only (alone, or on another space: AZD_ERR_INVALID_ARGUMENT naming the argument): the same cost up to
 * 64 vertices, the dense-graph space's own limit -- the device procedure with 64 rows (a wave's packed triangle is 2080 doubles,
 * 16.6 KB of LDS, where the 32-row form's is 4.1 KB), in kernels of their own; the 32-row kernels and every engine without the flag
 * are what they are without it.  Never chosen from the sizes.  Limits: 4 <= n <= AZD_DENSE_AH_WIDE_MAX_N, layers <= 1, ActionSet
 * paths, max_slots <= min(E, 640) (key widths 2, 4 and 10; roots of more than 640 slots are out of scope).  A wide engine on
 * n <= 32 is accepted and gives the trees the narrow engine gives.  eval = slope * (cost + 2.0f), slope = 1.0f / (2n + 2), as
 * there.  Its argmin record is azd_dense_ah_wide_argmin, read with azd_engine_dense_ah_wide_argmin_data
 * (azd_engine_dense_ah_argmin_data is AZD_ERR_UNSUPPORTED on it and names that call); azd_engine_dense_ah_agent_cost serves both.
 * Pool step: a searcher wave's LDS block is 20 KB, so a searcher workgroup has as many wavefronts as a CU's 160 KB hold -- 6 --
 * where the narrow engine's has 7..10 and the default cost's 16 (azd_debug_ext_pool_plan reports the plan for such a
 * configuration too); AZD_DENSE_POOL_WAVES keeps its range 4..16, a setting above what fits runs what fits. */
#define AZD_ENGINE_DENSE_AH_WIDE 256u
/* The dense-graph space with the weighted-invariant cost (azd_dense_inv_cost below): ten graph invariants combined with weights
 * given at RUN time by azd_engine_set_dense_inv_recipe, so that one build serves a family of objectives.  A tier of its own, in
 * kernels of their own (dense_inv_kernels.hip); asked for by name, never inferred.  In every respect but its cost it behaves as an
 * AZD_ENGINE_DENSE_AH engine: 4 <= n <= AZD_DENSE_INV_MAX_N = 32, layers <= 1, max_slots <= E, ActionSet paths (refused by
 * azd_engine_create with AZD_ERR_INVALID_ARGUMENT and an azd_last_error() naming the argument, as is this flag beside
 * AZD_ENGINE_DENSE_AH or AZD_ENGINE_DENSE_AH_WIDE or on another space); the same step forms, the pool step's wave counts (10 / 9 / 7
 * at key widths 2 / 4 / 10), AZD_ENGINE_EXT_POOL_F32 accepted beside it.  Such an engine keeps the ten invariants, the distance
 * index used and the `computed` mask per agent; read them with azd_engine_dense_inv_agent_cost and
 * azd_engine_dense_inv_argmin_data (the default and the AH argmin reads, and azd_engine_agent_state's lambda_1 / matching_size, are
 * AZD_ERR_UNSUPPORTED on it and name the right call). */
#define AZD_ENGINE_DENSE_INV 1024u
/* Beside AZD_ENGINE_DENSE_INV only (alone, beside AZD_ENGINE_DENSE_AH or AZD_ENGINE_DENSE_AH_WIDE, or on another space:
 * AZD_ERR_INVALID_ARGUMENT naming the argument): the weighted-invariant cost up to 64 vertices, the dense-graph space's own limit
 * -- the device procedure with 64 rows (one packed triangle of 2080 doubles serves both spectral passes), in kernels of their own
 * (dense_inv_wide_kernels.hip); the 32-row kernels and every engine without the flag are what they are without it.  Never chosen
 * from the sizes.  Limits: 4 <= n <= AZD_DENSE_INV_WIDE_MAX_N, layers <= 1, ActionSet paths, 1 <= max_slots <= min(E, 640) (key
 * widths 2, 4 and 10; roots of more than 640 slots are out of scope); AZD_ENGINE_EXT_POOL_F32 is accepted beside it.  A wide
 * engine on n <= 32 is accepted and gives the trees the narrow engine gives; under the Aouchiche-Hansen recipe it gives the trees
 * of an AZD_ENGINE_DENSE_AH_WIDE engine.  azd_engine_set_dense_inv_recipe (indices checked against 0 .. n - 1 at the engine's n) and
 * azd_engine_dense_inv_agent_cost serve both tiers.  Its argmin record is azd_dense_inv_wide_argmin, read with
 * azd_engine_dense_inv_wide_argmin_data (azd_engine_dense_inv_argmin_data is AZD_ERR_UNSUPPORTED on it and names that call, and
 * the reverse).  Pool step: a searcher wave's LDS block is the AZD_ENGINE_DENSE_AH_WIDE tier's, so a searcher workgroup has the 6
 * wavefronts it has there (azd_debug_ext_pool_plan reports the plan for such a configuration too). */
#define AZD_ENGINE_DENSE_INV_WIDE 2048u
/* The dense-graph space with the extended invariant cost (azd_dense_invx_cost below): sixteen invariants -- the weighted-invariant
 * cost's ten, one eigenvalue each of the Laplacian and the signless Laplacian, the Randic index, both Zagreb indices, the triangle
 * count -- combined by a recipe of weights and up to four products or quotients of two invariants, given at RUN time by
 * azd_engine_set_dense_invx_recipe.  A tier of its own beside AZD_ENGINE_DENSE_INV, in kernels of their own
 * (dense_invx_kernels.hip); asked for by name, never inferred.  It has that tier's limits, step forms and pool-step wave counts:
 * 4 <= n <= AZD_DENSE_INVX_MAX_N = 32, layers <= 1, max_slots <= E, ActionSet paths (refused with AZD_ERR_INVALID_ARGUMENT naming
 * the argument, as is this flag beside AZD_ENGINE_DENSE_AH, AZD_ENGINE_DENSE_AH_WIDE, AZD_ENGINE_DENSE_INV or
 * AZD_ENGINE_DENSE_INV_WIDE, or on another space); AZD_ENGINE_EXT_POOL_F32 is accepted beside it.  Such an engine keeps the sixteen
 * invariants, the distance index used and the `computed` mask per agent: azd_engine_dense_invx_agent_cost,
 * azd_engine_dense_invx_argmin_data.  The INV, AH and default reads and the INV setter are AZD_ERR_UNSUPPORTED on it and name the
 * right call, and the INVX calls on an AZD_ENGINE_DENSE_INV engine likewise. */
#define AZD_ENGINE_DENSE_INVX 4096u
/* Beside AZD_ENGINE_DENSE_INVX only (alone, beside any AZD_ENGINE_DENSE_AH* or AZD_ENGINE_DENSE_INV* flag, or on another space:
 * AZD_ERR_INVALID_ARGUMENT naming the argument): the extended invariant cost up to 64 vertices, the dense-graph space's own limit
 * -- the device procedure with 64 rows (one packed triangle of 2080 doubles serves the four spectral passes), in kernels of their
 * own (dense_invx_wide_kernels.hip); the 32-row kernels and every engine without the flag are what they are without it.  Never
 * chosen from the sizes.  Limits: 4 <= n <= AZD_DENSE_INVX_WIDE_MAX_N, layers <= 1, ActionSet paths, 1 <= max_slots <= min(E, 640)
 * (key widths 2, 4 and 10; roots of more than 640 slots are out of scope); AZD_ENGINE_EXT_POOL_F32 is accepted beside it.  A wide
 * engine on n <= 32 is accepted and gives the trees the narrow engine gives; under a weighted-invariant recipe it gives the trees
 * of an AZD_ENGINE_DENSE_INV_WIDE engine.  azd_engine_set_dense_invx_recipe (indices checked against 0 .. n - 1 at the engine's n)
 * and azd_engine_dense_invx_agent_cost serve both tiers.  Its argmin record is azd_dense_invx_wide_argmin, read with
 * azd_engine_dense_invx_wide_argmin_data (azd_engine_dense_invx_argmin_data is AZD_ERR_UNSUPPORTED on it and names that call, and
 * the reverse; the INV, AH and default reads likewise).  Pool step: a searcher wave's LDS block is the AZD_ENGINE_DENSE_AH_WIDE
 * tier's, so a searcher workgroup has the 6 wavefronts it has there (azd_debug_ext_pool_plan reports the plan for such a
 * configuration too). */
#define AZD_ENGINE_DENSE_INVX_WIDE 8192u
/* The dense-graph space with the spectrum invariant cost (azd_dense_invs_cost below): twenty-one invariants -- the extended
 * invariant cost's sixteen, then the graph energy, the distance energy, the Laplacian and signless-Laplacian energies and the
 * adjacency spread, each a function of a matrix's WHOLE spectrum -- combined by a recipe of weights and up to four products or
 * quotients of two invariants, given at RUN time by azd_engine_set_dense_invs_recipe.  A tier of its own beside
 * AZD_ENGINE_DENSE_INVX, in kernels of their own (dense_invs_kernels.hip); asked for by name, never inferred from a recipe.  It has
 * that tier's limits: 4 <= n <= AZD_DENSE_INVS_MAX_N = 32, layers <= 1, max_slots <= E,
 * ActionSet paths (refused with AZD_ERR_INVALID_ARGUMENT naming the argument, as is this flag beside any AZD_ENGINE_DENSE_AH*,
 * AZD_ENGINE_DENSE_INV* or AZD_ENGINE_DENSE_INVX* flag, or on another space).  Its 64-row form is asked for by AZD_ENGINE_DENSE_INVS_WIDE beside it.  There is, for now, no pool
 * step: its engines run one launch per phase at every population; AZD_ENGINE_EXT_POOL_F32 is accepted beside it and changes
 * nothing, and azd_debug_ext_pool_plan is AZD_ERR_UNSUPPORTED for such a configuration.  Such an engine keeps the twenty-one invariants, the distance index used and the `computed` mask per
 * agent: azd_engine_dense_invs_agent_cost, azd_engine_dense_invs_argmin_data.  The INVX, INV, AH and default reads and the INV and
 * INVX setters are AZD_ERR_UNSUPPORTED on it and name the right call, and the INVS calls on an engine of those tiers likewise. */
#define AZD_ENGINE_DENSE_INVS 16384u
/* Beside AZD_ENGINE_DENSE_INVS only (alone, beside any AZD_ENGINE_DENSE_AH*, AZD_ENGINE_DENSE_INV* or AZD_ENGINE_DENSE_INVX* flag, or
 * on another space: AZD_ERR_INVALID_ARGUMENT naming the argument): the spectrum invariant cost up to 64 vertices, the dense-graph
 * space's own limit -- the device procedure with 64 rows (one packed triangle of 2080 doubles serves the four spectral passes; at
 * n = 64 every lane of the wave owns an eigenvalue of the whole-spectrum finisher), in kernels of their own
 * (dense_invs_wide_kernels.hip); the 32-row kernels and every engine without the flag are what they are without it.  Never chosen
 * from the sizes.  Limits: 4 <= n <= AZD_DENSE_INVS_WIDE_MAX_N, layers <= 1, ActionSet paths, 1 <= max_slots <= min(E, 640) (key
 * widths 2, 4 and 10; roots of more than 640 slots are out of scope).  A wide engine on n <= 32 is accepted and gives the trees the
 * narrow engine gives; under an extended-invariant recipe it gives the trees of an AZD_ENGINE_DENSE_INVX_WIDE engine.
 * azd_engine_set_dense_invs_recipe (indices checked against 0 .. n - 1 at the engine's n) and azd_engine_dense_invs_agent_cost
 * serve both tiers.  Its argmin record is azd_dense_invs_wide_argmin, read with azd_engine_dense_invs_wide_argmin_data
 * (azd_engine_dense_invs_argmin_data is AZD_ERR_UNSUPPORTED on it and names that call, and the reverse; the INVX, INV, AH and
 * default reads likewise).  No pool step, as on the narrow tier: one launch per phase at every population,
 * AZD_ENGINE_EXT_POOL_F32 is accepted and changes nothing, azd_debug_ext_pool_plan is AZD_ERR_UNSUPPORTED. */
#define AZD_ENGINE_DENSE_INVS_WIDE 32768u
/* Beside AZD_ENGINE_RAMSEY_U64 only (alone, on another space or on a 32-bit tier: AZD_ERR_INVALID_ARGUMENT naming both flags): the
 * 64-bit tier with forbidden cliques up to K8 -- clique sizes 2..AZD_RAMSEY_BIG_CLIQUE_MAX, the reference's count_cliques_inside
 * (bitset_graph/mod.rs:164-185) to depth 6 in kernels of their own; the 64-bit tier's kernels and every engine without the flag are
 * what they are without it, a size 6 included ("clique sizes 2..5").  Never chosen from the sizes.  Every other limit is the
 * 64-bit tier's (3 <= n <= 64, 2..4 colours, E*C <= 2304, the max_slots rules, ActionSet paths, no Layered wrapper), and so are the
 * step forms (launch per phase, or the searcher-only pool step beside AZD_ENGINE_EXT_POOL_STEP / AZD_ENGINE_EXT_POOL_F32), the root
 * policy and the read-back entries (azd_engine_ramsey_argmin_any).  One limit more, the reference's own: RamseyCounts::new
 * (ramsey_counts/mod.rs:47-62) adds a colour's per-edge counts into an i32 before it divides by C(s,2), so every colour needs
 * C(s,2) * C(n,s) <= 2^31 - 1 -- size 6 at every n <= 64, size 7 at n <= 50, size 8 at n <= 39; azd_last_error() names the colour.
 * Shapes the 64-bit tier takes without the flag give the same trees with it. */
#define AZD_ENGINE_RAMSEY_BIG_CLIQUES 512u
/* AZD_SPACE_RAMSEY with max_slots > 0 only (the 32-bit wide tier, or the 64-bit tier beside AZD_ENGINE_RAMSEY_U64): the
 * searcher-only pool step, the CU-resident form of these engines for a model that does not fit an evaluator workgroup's LDS.
 * Persistent searcher workgroups of eight wavefronts pull agents from the per-XCD ready queues, write each new node's state row
 * to memory (f32, and bf16 beside it for a bf16 model) and post a request; on a second stream the host replays a graph of [collect
 * the requests, the model's GEMMs over the gathered rows, hand the agents back] for as long as the searchers run -- the dense-graph
 * space's form.  Results are bit for bit those of the launch-per-phase form.  Never chosen from the sizes: without the flag every
 * engine, limit, kernel, fallback chain and reason string is what it is without it.  On any other engine (c21, dense-graph,
 * Ramsey with max_slots == 0) and together with AZD_ENGINE_NO_PERSISTENT_STEP azd_engine_create returns
 * AZD_ERR_INVALID_ARGUMENT.  Needs an evaluator that serves gathered bf16 rows: an MLP with AZD_STORAGE_BF16 (or the tests' hash
 * stream) -- or, beside AZD_ENGINE_EXT_POOL_F32 below, an MLP with AZD_STORAGE_F32; with any other the engine runs what it would have run without the flag and azd_engine_step_form's reason opens with
 * "external pool step:".  When the form runs azd_engine_step_form reports AZD_STEP_POOL with an empty reason and
 * azd_engine_pool_split 0 evaluator workgroups beside the searcher workgroups.
 * Which form where (profiles/r09_ramsey_ext_pool.txt, bf16 storage): on the 64-bit tier this one -- 1.5 times the launch-per-phase
 * form at r3333, 3.3 times at r45.  On the 32-bit wide tier prefer the in-kernel pool step (AZD_ENGINE_POOL_STEP, the default from
 * 256 agents) wherever its plan takes the model: at r45 with 512-1024-512 the two run level (1.39 against 1.40 M expansions/s, 256
 * agents) and the in-kernel form needs no second stream and no host thread; take this one for a model whose 16 bf16 rows of
 * activations do not fit an evaluator workgroup's LDS, where the in-kernel form falls back to one launch per phase (0.39 M). */
#define AZD_ENGINE_EXT_POOL_STEP 64u
/* Beside AZD_ENGINE_EXT_POOL_STEP on the Ramsey tiers (alone there, and on c21: AZD_ERR_INVALID_ARGUMENT from azd_engine_create and
 * azd_debug_ext_pool_plan, naming both flags), ALONE on AZD_SPACE_DENSE (below): the
 * form also takes an MLP with fp32 storage (AZD_STORAGE_F32, the reference's own models).  The searchers are the same -- they
 * write the f32 row whatever the model -- and the evaluator's graph runs the layers as gathered fp32 GEMMs on
 * v_mfma_f32_32x32x2_f32 over those rows: every prediction is the sum azd_evaluator_write_predictions gives the row, bit for bit,
 * so results are those of the launch-per-phase form.  The LDS plan is that of AZD_ENGINE_EXT_POOL_STEP alone.  With a bf16 model
 * nothing differs from AZD_ENGINE_EXT_POOL_STEP alone; without this flag an fp32 model under AZD_ENGINE_EXT_POOL_STEP keeps
 * falling back with the "external pool step: ... bf16" reason.  A storage switch (azd_evaluator_set_weight_storage) re-captures
 * the evaluator's graph.  Measured (profiles/r10_ramsey_ext_f32.txt, fp32, against the launch-per-phase form on the same box): r3333 at
 * 512 agents 0.99 against 0.52 M expansions/s, r45 at 256 agents 1.03 against 0.31 M on the wide tier and 0.79 against 0.25 M on the
 * 64-bit tier.
 * AZD_SPACE_DENSE: the space's pool step is the searcher-only form and needs no flag of its own, so there this flag stands alone, on
 * all eight tiers (default cost, AZD_ENGINE_DENSE_AH, AZD_ENGINE_DENSE_AH_WIDE, AZD_ENGINE_DENSE_INV, AZD_ENGINE_DENSE_INV_WIDE, AZD_ENGINE_DENSE_INVX, AZD_ENGINE_DENSE_INVX_WIDE; AZD_ENGINE_DENSE_INVS, with or without AZD_ENGINE_DENSE_INVS_WIDE, accepts the flag but has no pool step); AZD_ENGINE_EXT_POOL_STEP stays refused there, and
 * this flag beside AZD_ENGINE_NO_PERSISTENT_STEP is AZD_ERR_INVALID_ARGUMENT naming both.  It is a request to the configured pool
 * step, not a form: where the engine's form is not the pool step (fewer than 256 agents without AZD_ENGINE_POOL_STEP) nothing
 * changes and azd_engine_step_form gives the reason it gave.  With it an fp32 MLP is served by the same gathered fp32 GEMMs over the
 * engine's f32 state rows, on the plan a bf16 model gets (same wavefronts per workgroup, LDS bytes and workgroups;
 * azd_debug_ext_pool_plan takes a dense configuration with the flag); without it an fp32 MLP keeps falling back with "dense-graph
 * space: the pool step needs an evaluator that serves gathered bf16 rows"; with it and an evaluator that serves no rows at all the
 * reason opens with "dense-graph space:" too.  Measured on one MI355X (profiles/r16_dense_ext_f32.txt; fp32, whole epochs of 200
 * calls in one launch, against the launch-per-phase form): AH N = 31 (1396-256-128-930) 2.62 against 0.82 M expansions/s at 512
 * agents and 5.51 against 4.69 M at 4096; AH-wide N = 50 at 512 agents 1.51 against 0.55 M.  NOT everywhere a gain: at BASELINE
 * configs[4]'s shape (N = 50, 512-512-512, 8192 agents) the evaluator's stream is busy 0.99 of the launch and the form runs 4.04
 * against 6.80 M (roots of at most 612 slots: 4.03 against 5.55 M) -- at that population one whole-batch fp32 GEMM per call beats
 * gathered batches; and with ONE call per launch (examples/ah.py's loop) 0.49 against 0.57 M.  One evaluator stream, as for bf16
 * (AZD_DENSE_POOL_STREAMS=2: +2..4 % at 512 agents, -9 % at 4096). */
#define AZD_ENGINE_EXT_POOL_F32 128u

/* ArgminData<State, Cost> (az-discrete-opt/src/log.rs:1-11) for the c21 space */
typedef struct azd_argmin {
    uint8_t parents[32];
    uint64_t permitted[4];
    double lambda_1;           /* Conjecture2Dot1Cost.lambda_1 */
    int32_t matching_size;     /* Conjecture2Dot1Cost.matching.len() */
    int32_t matching[32];      /* (parent, child) pairs of the matching */
    float eval;
    int32_t agent;             /* tree the state was found in */
    uint32_t node;             /* its node index in that tree */
} azd_argmin;

/* ArgminData<RamseyCountsNoRecolor, TotalCounts<C>> for the Ramsey space */
typedef struct azd_ramsey_argmin {
    uint8_t colors[256];       /* colour per colex edge position */
    uint64_t permitted[4];     /* permitted edge positions */
    int32_t totals[4];         /* TotalCounts: monochromatic cliques per colour */
    float eval;
    int32_t agent;
    uint32_t node;
} azd_ramsey_argmin;

/* The same for any Ramsey engine, wide ones included (N <= 32: E <= 496 edges) */
typedef struct azd_ramsey_wide_argmin {
    uint8_t colors[496];       /* colour per colex edge position (E of them) */
    uint64_t permitted[8];     /* permitted edge positions */
    int32_t totals[4];         /* TotalCounts: monochromatic cliques per colour */
    float eval;
    int32_t agent;
    uint32_t node;
} azd_ramsey_wide_argmin;

/* ArgminData for the dense-graph space: the graph, its open slots, Conjecture2Dot1Cost */
typedef struct azd_dense_argmin {
    uint64_t adj[64];
    uint64_t permitted[40];    /* BITMAP over the E edge slots (colex positions) still modifiable: (E + 63) / 64 words
                                * (32 at AZD_DENSE_MAX_N), NOT an action-id set of azd_dense_key_words() words */
    double lambda_1;
    int32_t matching_size;
    float eval;
    int32_t agent;
    uint32_t node;
} azd_dense_argmin;

enum { /* indices into azd_engine_counters' output */
    AZD_CTR_EXPANSIONS = 0,     /* calls that ended on a new non-terminal node (metric numerator) */
    AZD_CTR_TERMINALS = 1,
    AZD_CTR_TRANSPOSITIONS = 2,
    AZD_CTR_VISITED_STEPS = 3,
    AZD_CTR_SELECT_CALLS = 4,
    AZD_CTR_SUM_DEG = 5,
    AZD_CTR_SUM_ACTIONS = 6,
    AZD_CTR_CASCADE_NODES = 7,
    AZD_CTR_NEW_PREDS = 8,
    AZD_CTR_ROOT_EXHAUSTED = 9,
    AZD_CTR_MAX_FRONTIER = 10,
    AZD_CTR_MAX_DEPTH = 11,
    AZD_CTR_CURIOSITY_PAIRS = 12,
    AZD_CTR_EVAL_LAYER_CLOCKS = 13, /* pool step: shader clocks the evaluator workgroups spent in the MLP's layers, summed (s_memtime); with
                                     * slot 31's 100 MHz ticks of the same spans it gives the clock the evaluator CUs actually held */
    AZD_CTR_TICKS_ADD_ACTIONS = 14, /* pool step, AZD_WAVE_PHASES builds: ticks from an agent taken to its arrived row's actions added */
    AZD_CTR_FAILED_AGENTS = 15,
    /* 16..22: 100 MHz ticks per phase of the roll-out kernel, summed over agents; filled only by
     * the diagnostic build (make PROFILE=1), 0 otherwise */
    AZD_CTR_TICKS_TOTAL = 16,
    AZD_CTR_TICKS_SELECT = 17,
    AZD_CTR_TICKS_LOOKUP = 18,
    AZD_CTR_TICKS_NEWNODE = 19,
    AZD_CTR_TICKS_CASCADE = 20,
    AZD_CTR_TICKS_MAX_CALL = 21, /* max over agents and calls of one agent's ticks in one call */
    AZD_CTR_TICKS_LAMBDA = 22,   /* inside NEWNODE: lambda_1 */
    AZD_CTR_TICKS_MATCHING = 23, /* inside NEWNODE: matching */
    AZD_CTR_TICKS_WAIT = 24,     /* waiting for / serving the in-kernel evaluator */
    /* evaluator service of the asynchronous step (always counted) */
    AZD_CTR_EVAL_BATCHES = 25,
    AZD_CTR_EVAL_ROWS = 26,
    AZD_CTR_EVAL_TILES = 27,
    AZD_CTR_TICKS_TILES = 28,   /* diagnostic build: ticks inside evaluator tile tasks */
    AZD_CTR_TICKS_BATCH = 29,   /* pool step, every build: 100 MHz ticks from batch taken to batch released, summed over the evaluator
                                 * workgroups (bench.py's evaluator_weight_stream / us_per_batch read it); the asynchronous step fills it
                                 * in the diagnostic build only */
    AZD_CTR_COUNT = 32
};

/* Allocates the device arenas.  `ev` may be NULL (external evaluator: drive the
 * engine with the *_begin/_end pairs and supply predictions yourself). */
int azd_engine_create(azd_engine **out, const azd_engine_config *cfg, azd_evaluator *ev);
int azd_engine_destroy(azd_engine *e);

/* NablaOptimizer::par_new (optimizer/mod.rs:39-118).  `init_states` stays on the
 * host: the caller passes the packed roots it produced. */
int azd_engine_par_new(azd_engine *e, const uint8_t *parents, const uint64_t *permitted);
/* NablaOptimizer::par_roll_out_episodes (optimizer/mod.rs:121-191), `n_calls`
 * times back to back without a host round trip.  n_as_tol crosses the ABI as
 * table + default (04-c21-tree.rs:136-138).  *improved = number of calls that
 * returned ArgminImprovement::Improved. */
int azd_engine_par_roll_out_episodes(azd_engine *e, const uint32_t *n_as_tol, int n_tol,
                                     uint32_t n_as_tol_default, int n_calls, int *improved);
/* Run-ahead window, for a host that asks for its episodes ONE CALL AT A TIME as the reference's drivers do
 * (04-c21-tree.rs:142-150: par_roll_out_episodes, then a look at the ArgminImprovement, `episodes` times per epoch): a
 * launch of the CU-resident step costs ~0.6 ms whatever it holds, so 800 launches of one call run at a fifth of the speed
 * of one launch of 800.  azd_engine_run_ahead starts the next `n_calls` calls NOW, in one launch, and returns at once;
 * the azd_engine_par_roll_out_episodes calls that follow (same n_as_tol; one call or any chunk at a time) launch nothing:
 * each waits until the kernel has published the calls it asks for -- a call is published when its last agent is through it
 * -- and returns their ArgminImprovements exactly as separate launches would have.  azd_engine_argmin_data (and the Ramsey
 * form) inside the window return the record as of the calls handed out so far; the winner's replay reads its tree, so they
 * wait for the launch first.  Any other engine call closes the window: it waits for the launch, and the calls that were not
 * asked for have run and stay run (counters and trees show them).  The evaluator must not be updated by calls of its own
 * while a window is open (azd_engine_par_update_model closes it like every engine call).
 * *accepted = 0 when this engine's step cannot publish calls while it runs (any form but the pool step; n_calls beyond one
 * launch, 1024; per-launch timing on): nothing is started then and the calls run when they are asked for, so a host may
 * call this unconditionally. */
int azd_engine_run_ahead(azd_engine *e, const uint32_t *n_as_tol, int n_tol, uint32_t n_as_tol_default, int n_calls,
                         int *accepted);
/* NablaOptimizer::par_update_model (optimizer/mod.rs:249-281) */
int azd_engine_par_update_model(azd_engine *e, uint32_t n_obs_tol, float *loss);
/* par_update_model for a population SHARDED over several GPUs (one engine per process and GPU, contiguous agent
 * ranges in rank order; the reference has no such form -- optimizer/mod.rs:249-281 on one device): the training
 * triple of this rank (optimizer/mod.rs:262-278) is all-gathered over RCCL on the engine's stream into
 * engine-owned buffers, then every rank takes the identical optimiser step on the pooled batch*world rows (the
 * loss normaliser sum(w) is global over the batch, model/dfdx.rs:106,110).  `nccl_comm` is the caller's ncclComm_t
 * (ncclCommInitRank on this engine's device); the evaluator must have been created with max_batch >= batch*world.
 * librccl.so is bound at first use; AZD_ERR_UNSUPPORTED if it cannot be loaded. */
int azd_engine_par_update_model_sharded(azd_engine *e, uint32_t n_obs_tol, void *nccl_comm, float *loss);
/* NablaOptimizer::par_reset_trees (optimizer/mod.rs:284-360) with the
 * `modify_root` closure applied by the caller (see azd_c21_modify_roots). */
int azd_engine_par_reset_trees(azd_engine *e, const uint8_t *parents, const uint64_t *permitted);
/* NablaOptimizer::argmin_data (optimizer/mod.rs:361) */
int azd_engine_argmin_data(azd_engine *e, azd_argmin *out);
int azd_engine_ramsey_argmin_data(azd_engine *e, azd_ramsey_argmin *out); /* AZD_SPACE_RAMSEY engines with E <= 256 */
int azd_engine_ramsey_wide_argmin_data(azd_engine *e, azd_ramsey_wide_argmin *out); /* AZD_SPACE_RAMSEY engines with E <= 496 */
/* The same for EVERY Ramsey engine, with the caller's capacities instead of a fixed-size record: `colors` receives E bytes
 * (colors_cap >= E), `permitted` (E + 63) / 64 words (permitted_words_cap >= that); what lies beyond is zeroed.  totals[4].  Any
 * output pointer may be NULL. */
int azd_engine_ramsey_argmin_any(azd_engine *e, uint8_t *colors, int colors_cap, uint64_t *permitted, int permitted_words_cap,
                                 int32_t *totals, float *eval, int32_t *agent, uint32_t *node);
int azd_engine_dense_argmin_data(azd_engine *e, azd_dense_argmin *out);   /* AZD_SPACE_DENSE engines */
/* the agent's live per-edge clique counts [C][E] and totals [4] (RamseyCounts, mod.rs:12-17) */
int azd_engine_ramsey_agent_counts(azd_engine *e, int agent, int32_t *counts, int32_t *totals);

/* The `modify_root` policy of the c21 driver (04-c21-tree.rs:172-206), seeded;
 * reads each tree's node_data() (tree/mod.rs:302-307) and writes new packed roots. */
int azd_c21_modify_roots(azd_engine *e, uint64_t seed, uint64_t epoch, int kmin, int kmax,
                         uint8_t *parents_out, uint64_t *permitted_out);

/* The same policy evaluated on the device (one wavefront per tree, radix select of the chosen key
 * in BTreeMap order): _dev returns the roots it would install, par_reset_trees_c21 = policy +
 * par_reset_trees with no host round trip. */
int azd_c21_modify_roots_dev(azd_engine *e, uint64_t seed, uint64_t epoch, int kmin, int kmax,
                             uint8_t *parents_out, uint64_t *permitted_out);
int azd_engine_par_reset_trees_c21(azd_engine *e, uint64_t seed, uint64_t epoch, int kmin, int kmax);
/* The Ramsey drivers' modify_root (02-r44.rs:196-228) is the same policy over permitted EDGES
 * (k' of the E edges instead of k' of ACTION_DIM; a fresh root is a fresh random colouring), and
 * the device kernel serves both spaces.  Space-neutral names of the two calls above: */
int azd_engine_modify_roots_dev(azd_engine *e, uint64_t seed, uint64_t epoch, int kmin, int kmax,
                                uint8_t *roots_out, uint64_t *permitted_out);
int azd_engine_par_reset_trees_policy(azd_engine *e, uint64_t seed, uint64_t epoch, int kmin, int kmax);

/* What the device policy of the four calls above does at the epoch boundary: engine state, set between any two engine calls.
 *   rule           which nodes an IMPROVED tree (c_root != c_root_star) keeps before one is picked uniformly:
 *                  THRESHOLD c <= (c_root + 3 c_root_star) / 4, or BEST c == c_root_star.  The stagnant branch, the draws and
 *                  the shuffle are the same under both.
 *   color_weights  AZD_SPACE_RAMSEY: the colours of a FRESH root (azd_ramsey_generate_roots_weighted's thresholds over the
 *                  policy's own draws); n_color_weights = 0: uniform, else = the engine's n_colors.
 * Refused with AZD_ERR_INVALID_ARGUMENT and an azd_last_error() that names the field: an unknown rule; colour weights on an
 * engine of another space; n_color_weights other than 0 and n_colors; a weight that is not finite and positive.
 * p = NULL sets the defaults {THRESHOLD, no weights}, with which every root is what it was before this call existed.
 * azd_engine_get_root_policy(NULL, p) writes those defaults.  azd_root_policy_check is the check alone, without an engine. */
#define AZD_ROOT_RULE_THRESHOLD 0 /* 02-r44.rs:194-196, 04-c21-tree.rs:196-198: the default */
#define AZD_ROOT_RULE_BEST 1      /* 05-r45.rs:201, 03-r3333.rs:191: keep c == c_root_star */
typedef struct {
    int rule;
    int n_color_weights;
    double color_weights[4];
} azd_root_policy;
int azd_engine_set_root_policy(azd_engine *e, const azd_root_policy *p);
int azd_engine_get_root_policy(const azd_engine *e, azd_root_policy *p);
int azd_root_policy_check(int space_id, int n_colors, const azd_root_policy *p);
/* What the last policy evaluation (any of the four calls) did with each tree; [batch] each, any pointer may be NULL:
 *   branch  0 a fresh root, 1 stagnant (c_root == c_root_star: grow the permitted set), 2 improved (jump to a kept node)
 *   node    the chosen node's index in the tree it was chosen from (0xFFFFFFFF for a fresh root)
 *   kept    the size of the set it was chosen from (0 for a fresh root)
 * AZD_ERR_INVALID_ARGUMENT before any evaluation.  An empty kept set -- the reference's unwrap() on None; it cannot happen,
 * c_root_star is some node's cost -- makes the policy call itself return AZD_ERR_UNREACHABLE. */
int azd_engine_root_policy_report(azd_engine *e, uint8_t *branch, uint32_t *node, uint32_t *kept);

/* Split-phase forms of the three calls above, cut at the model call
 * (optimizer/mod.rs:72, :175-176, :348), for an external NablaModel:
 * *_begin leaves the state vectors ready, *_end consumes h_theta (host, batch*action_dim). */
int azd_engine_par_new_begin(azd_engine *e, const uint8_t *parents, const uint64_t *permitted);
int azd_engine_par_new_end(azd_engine *e, const float *h_theta);
int azd_engine_roll_out_begin(azd_engine *e, const uint32_t *n_as_tol, int n_tol,
                              uint32_t n_as_tol_default);
int azd_engine_roll_out_end(azd_engine *e, const float *h_theta, int *improved);
int azd_engine_reset_begin(azd_engine *e, const uint8_t *parents, const uint64_t *permitted);
int azd_engine_reset_end(azd_engine *e, const float *h_theta);
/* par_update_model without the model call: fills the training triple
 * (optimizer/mod.rs:262-278).  Host copies (any may be NULL) ... */
int azd_engine_observe(azd_engine *e, uint32_t n_obs_tol, float *state_vecs, float *observations,
                       float *action_weights);
/* ... or the device buffers themselves, for an all-gather across GPUs. */
int azd_engine_observe_dev(azd_engine *e, uint32_t n_obs_tol, const float **d_state_vecs,
                           const float **d_observations, const float **d_action_weights);
int azd_engine_read_state_vecs(azd_engine *e, float *state_vecs); /* batch*state_dim */
int azd_engine_read_predictions(azd_engine *e, float *h_theta);   /* last h_theta, batch*action_dim */
/* Test entry: `rows` prediction rows exactly as the CU-resident step forms' in-kernel evaluator computes them (the same sums in
 * the same order; the model call of model/dfdx.rs:69-84), for state vectors the host hands over: what a checker feeds its
 * restatement with to follow a whole launch of the product kernel with the real model.  c21 / Ramsey space, MLP evaluator
 * (f32 or bf16 storage). */
int azd_engine_debug_tile_forward(azd_engine *e, const float *states, float *predictions, int rows);

/* Introspection (SearchTree::{nodes, positions, node_data}, tree/mod.rs:302-315;
 * get_trees, optimizer/mod.rs:34-36): raw arrays instead of graphviz. */
int azd_engine_tree_sizes(azd_engine *e, int agent, int *n_nodes, int *n_arcs, int *n_predictions);
int azd_engine_export_tree(azd_engine *e, int agent, float *c, float *c_star, uint32_t *n_t,
                           uint32_t *exhausted, uint32_t *act_begin, uint32_t *act_end,
                           uint64_t *keys, uint32_t *arc_src, uint32_t *arc_dst, uint32_t *arc_pp,
                           uint32_t *pred_a_id, float *pred_g, int32_t *pred_arc);
int azd_engine_agent_state(azd_engine *e, int agent, uint8_t *parents, uint64_t *permitted,
                           uint64_t *path, uint32_t *state_pos, double *lambda_1,
                           int *matching_size);
int azd_engine_counters(azd_engine *e, uint64_t *out /* [AZD_CTR_COUNT] */);
/* the same counters per agent, unreduced: out[batch][AZD_CTR_COUNT] (load-balance diagnostics).  The launch-per-phase and
 * asynchronous forms attribute every count to its agent.  The pool step of the product build adds a searcher wave's counts once,
 * when the wave leaves the launch, to ONE agent's block (the sums and maxima of azd_engine_counters are the same; the per-call
 * read-modify-write of the agent's block was a dependent round trip on the wave's time): per-agent attribution under the pool
 * step is the diagnostic build's (make PROFILE=1, tools/slow_agents.py). */
int azd_engine_agent_counters(azd_engine *e, uint64_t *out);
/* 1 while every block of azd_engine_agent_counters holds its own agent's counts; 0 once a pool launch of the product build has
 * run since the counters were last cleared (azd_engine_par_new): the blocks then hold what searcher waves counted and only their
 * sums / maxima (azd_engine_counters) mean anything.  Load-balance tools must check this before reading per-agent values. */
int azd_engine_agent_counters_per_agent(azd_engine *e);
/* ms of GPU time spent in the tree kernels / evaluator since creation (HIP events
 * on the engine's stream; enabled by azd_engine_set_timing) */
int azd_engine_set_timing(azd_engine *e, int enabled);
int azd_engine_timing(azd_engine *e, double *tree_ms, double *evaluator_ms, uint64_t *tree_launches);
void *azd_engine_stream(azd_engine *e); /* hipStream_t the engine launches on */
/* Which form of the step the last azd_engine_par_roll_out_episodes ran (identical results, very different
 * speed): the asynchronous CU-resident step, the lock-step CU-resident step, or one launch per phase and
 * call (external evaluators, models the in-kernel evaluator cannot take).  *reason (owned by the engine,
 * valid until the next call) says why a faster form was not taken, "" when the preferred one ran.
 * The pool step needs its searcher and evaluator workgroups resident together: the grid is clamped to what the occupancy query
 * reports, a device without room for one of each runs the asynchronous step, and a pool launch whose waits run into their
 * bound (4 s without progress) is TAKEN OVER by the asynchronous step where every agent stands -- same results, the call
 * succeeds, *reason says so and the engine stays with the asynchronous step (dense-graph space, whose evaluator runs beside the
 * kernel: completed by the launch-per-phase kernels in the same way, and the engine stays with those). */
#define AZD_STEP_NONE 0
#define AZD_STEP_ASYNC 1
#define AZD_STEP_BARRIER 2
#define AZD_STEP_PER_CALL 3
#define AZD_STEP_POOL 4
#define AZD_STEP_PER_CALL_GRAPH 5 /* AZD_STEP_PER_CALL with the launches of a call captured in a hipGraph and replayed */
int azd_engine_step_form(azd_engine *e, int *form, const char **reason);
/* how the last pool-step launch split the CUs: evaluator / searcher workgroups */
/* Evaluator groups of the last pool launch: `members` workgroups serve a batch together, each keeping the weight fragments of its
 * column tiles of every layer in LDS for the whole launch (no weight stream per batch; the batch's activations travel between the
 * layers through device memory), `groups` of them, a workgroup's waves in slots of `waves_per_slot`.  0 members: the classic form
 * (one workgroup per batch, weights streamed from L2).  The engine forms groups where a classic batch is long (fp32 weights beyond
 * 2.5 MB, at most 1536 agents: BASELINE configs[0], the reference's 304-512-1024-512-152); AZD_POOL_EVAL_GROUP = 0 / g overrides.
 * Same rows to the bit either way. */
int azd_engine_pool_groups(azd_engine *e, int *members, int *groups, int *waves_per_slot);
/* Pool step (product build): for every agent, when it was through with the calls of the LAST pool launch, in 100 MHz ticks from the
 * launch's first workgroup -- the launch lasts as long as its slowest agent's chain of calls (tree/mod.rs:113-232 is serial per
 * tree), so max over agents = the launch, and the distance of the median from it is what the epoch's barrier costs.
 * out[batch].  The diagnostic build (make PROFILE=1) uses the array for its own stamps: values are not finish times there. */
int azd_engine_pool_agent_finish(azd_engine *e, uint64_t *ticks_out);
int azd_engine_pool_split(azd_engine *e, int *eval_wgs, int *search_wgs);
/* ... and how busy its two sides were: the share of the launch an evaluator workgroup spent on batches, and the share a
 * searcher wave spent with an agent in hand (the engine moves the split towards equal shares from launch to launch) */
int azd_engine_pool_utilisation(azd_engine *e, double *eval_busy, double *search_busy);
/* HW_REG_XCC_ID read by every block of an n_blocks launch (the pool step keeps a tree on the XCD that first took it) */
int azd_debug_probe_xcc(int device, uint32_t *out, int n_blocks);
/* Test harness of the pool step: with `on`, a hash-stream evaluator's rows are served by the pool step's EVALUATOR workgroups
 * (through the queues, the early post and the join counter, like the MLP's) instead of by the searching wave itself, so that
 * whole launches of that machinery can be compared with the CPU oracle.  Same values either way.  Environment hooks of the
 * same harness: AZD_POOL_DEBUG_ABORT_CALL=k (agent 0 raises the launch's abort flag after its k-th call: the take-over by the
 * asynchronous step), AZD_POOL_MAX_RESIDENT=w (pretend the device holds w workgroups of the pool kernel at once). */
int azd_debug_hash_stream_via_evaluators(azd_evaluator *ev, int on);
/* The LDS plan of the searcher-only pool step (AZD_ENGINE_EXT_POOL_STEP; also a dense-graph configuration with
 * AZD_ENGINE_DENSE_AH_WIDE, whose pool step takes as many wavefronts as the LDS holds, and any dense-graph configuration with
 * AZD_ENGINE_EXT_POOL_F32, whose plan is the one a bf16 model gets: the flag is not read) for a configuration: wavefronts per
 * searcher workgroup and the bytes of LDS one workgroup takes (of the CU's 160 KB).  Arithmetic on the configuration: no device is
 * touched.  AZD_ERR_INVALID_ARGUMENT for a configuration azd_engine_create refuses, or one with none of these flags. */
int azd_debug_ext_pool_plan(const azd_engine_config *cfg, int *waves, size_t *lds_bytes);
/* The evaluator of the searcher-only pool step in isolation (tests): the MLP's gathered forward of whichever storage type it has
 * -- fp32: the gathered fp32 GEMMs of AZD_ENGINE_EXT_POOL_F32; bf16: the gathered bf16 GEMMs -- on host arrays.  states:
 * n_state_rows rows of state_dim floats; rows: n_rows (<= max_rows, the size the launches are made for) indices into them;
 * predictions: n_state_rows rows of action_dim floats, in and out: row rows[i] receives the prediction of state row rows[i],
 * every other row is left as it was.  AZD_ERR_UNSUPPORTED for evaluators other than the MLP. */
int azd_debug_write_predictions_gathered(azd_evaluator *ev, int max_rows, const uint32_t *rows, int n_rows, const float *states,
                                         int n_state_rows, float *predictions);
/* The MLP evaluator's training gradient without the optimiser step (tests against a float64 reference): the same launches
 * as azd_evaluator_update_model up to the Adam step, on host rows staged like that call's.  grads_out: num_params floats in
 * the get_params layout; *loss as update_model reports it.  Parameters, Adam moments and the step count are left untouched.
 * AZD_ERR_UNSUPPORTED for evaluators other than the MLP. */
int azd_debug_mlp_gradients(azd_evaluator *ev, int batch, const float *states, const float *observations,
                            const float *action_weights, float *grads_out, float *loss);

/* Parity probe for the two f32 primitives the selection rule (tree/next_action.rs:70,81) depends
 * on bit-for-bit.  in: 2*n floats (pairs x, y); out: 4*n floats per pair:
 * [0] the kernels' sqrt(|x - y|), [1] sqrtf, [2] __fsqrt_rn (diagnostics), [3] x - (x - y). */
int azd_debug_probe_math(int device, const float *in, float *out, int n);
/* c21 cost kernel in isolation (ordered_edge.rs:72-124): lambda_1 (full = 1: full f64 bracket as
 * ArgminData reports it; 0: the f32-exact early stop used for node costs) and the matching size of
 * `count` trees, one wavefront each, repeated `reps` times; *ms = GPU time of the timed launch. */
int azd_debug_probe_cost(int device, const uint8_t *parents, int n, int count, int reps, int full,
                         double *lambda_1, int *matching_size, float *ms);
/* The dense-graph space's default cost (Conjecture2Dot1Cost over general graphs: lambda_1 + matching number) in isolation, as the
 * search computes it: `count` graphs on n vertices (adj[count][n] neighbourhood bitsets), one wavefront each.  Step 0 is a root's
 * cost: lambda_1 and a maximum matching from nothing.  Step j = 1 .. n_toggles is a new node's: the edge at colex slot
 * toggles[g * n_toggles + j - 1] (slot of {v, u}, u < v: v (v - 1) / 2 + u) is added if absent and deleted if present, the
 * previous step's matching is repaired, lambda_1 is computed with a hook that counts its calls.  Outputs are
 * [count][n_toggles + 1]: lambda_1, matching_size, hook_calls (1 whenever the iteration keeps its contract), and mate as
 * [count][n_toggles + 1][64] bytes (the vertex's partner; 0xFF: unmatched, and at and above n).  Checked before the device is
 * looked for, with an azd_last_error() that names the graph: 4 <= n <= 64, count > 0, 0 <= n_toggles <= 64; every graph without
 * loops, symmetric, no bit at or above n; every slot below E = n (n - 1) / 2 and at most once per graph.  Connectivity is the
 * caller's business (a deletion may disconnect the graph: both procedures are defined there, the search never goes there). */
int azd_debug_probe_dense_cost(int device, const uint64_t *adj, int n, int count, const uint16_t *toggles, int n_toggles,
                               double *lambda_1, int *matching_size, uint8_t *mate, int *hook_calls);

/* ---- Aouchiche-Hansen cost: the dense-graph space's second objective (AZD_ENGINE_DENSE_AH engines minimise it; every other dense
 * engine minimises Conjecture2Dot1Cost = lambda_1 + matching number, as before). (the objective of the reference's examples/05-ah.rs,
 * ConnectedBitsetGraph::ah_cost, connected_bitset_graph/mod.rs:156-198).  For a CONNECTED graph on n vertices, from a BFS out of
 * every vertex: proximity pi = min_u sum_v d(u, v) / (n - 1); diameter D; k = floor(2D/3) - 1, or n - 1 when floor(2D/3) = 0
 * (complete graphs); eigenvalue = entry k (0-based) of the distance matrix's eigenvalues sorted descending;
 * cost = (float)(pi + eigenvalue).  A graph with cost < 0 would be a counterexample to the Aouchiche-Hansen conjecture.
 * BUILD-DEFINED (the reference's driver is a stub): eval = slope * (cost + 2.0f), slope = 1.0f / (2n + 2), in the image of the
 * dense space's squish; and the eigenvalue procedure that stands in for faer -- Householder tridiagonalisation, then a Sturm-count
 * multisection for the one eigenvalue -- one IEEE f64 operation at a time in a fixed order, so that this host function, the
 * device kernel (azd_debug_probe_ah_cost) and the tests' Python reference agree bit for bit (DESIGN.md "The AH cost").
 * 4 <= n <= AZD_DENSE_AH_MAX_N: at 32 vertices a wave's working matrix (a packed triangle) is 4 KB of LDS; at 64 it is 16.6 KB,
 * and that form has names of its own: AZD_DENSE_AH_WIDE_MAX_N, azd_dense_ah_cost_wide, AZD_ENGINE_DENSE_AH_WIDE. */
#define AZD_DENSE_AH_MAX_N 32
#define AZD_DENSE_AH_WIDE_MAX_N 64
typedef struct azd_dense_ah_cost_t {
    double proximity;  /* pi */
    double eigenvalue; /* entry k of the distance spectrum, descending */
    int32_t diameter;  /* D */
    int32_t k;
    float cost;        /* (float)(proximity + eigenvalue) */
    float eval;        /* slope * (cost + 2.0f) */
} azd_dense_ah_cost_t;
/* The cost on the host; needs no GPU.  adj: n neighbourhood bitsets (bit u of adj[v] = edge {u, v}).  AZD_ERR_INVALID_ARGUMENT
 * with an azd_last_error() that names the argument for n out of range or a graph that is not simple, symmetric and connected. */
int azd_dense_ah_cost(const uint64_t *adj, int n, azd_dense_ah_cost_t *out);
/* The same host function for 4 <= n <= AZD_DENSE_AH_WIDE_MAX_N: the same sequence of IEEE f64 operations and the same graph
 * checks; for n <= 32 bit for bit azd_dense_ah_cost. */
int azd_dense_ah_cost_wide(const uint64_t *adj, int n, azd_dense_ah_cost_t *out);
/* The device kernel in isolation: the cost of `count` graphs on n vertices (adj[count][n]), one wavefront each, repeated `reps`
 * times; *ms = GPU time of the timed launch.  The graphs are checked like azd_dense_ah_cost's, before the device is looked for. */
int azd_debug_probe_ah_cost(int device, const uint64_t *adj, int n, int count, int reps, azd_dense_ah_cost_t *out, float *ms);
/* ... and the 64-row kernel (AZD_ENGINE_DENSE_AH_WIDE engines' cost), 4 <= n <= AZD_DENSE_AH_WIDE_MAX_N; checked the same way */
int azd_debug_probe_ah_cost_wide(int device, const uint64_t *adj, int n, int count, int reps, azd_dense_ah_cost_t *out, float *ms);
/* ArgminData of an AZD_ENGINE_DENSE_AH engine: the graph, the slots still open, the cost's parts */
typedef struct azd_dense_ah_argmin {
    uint64_t adj[32];
    uint64_t permitted[8]; /* modifiable slots (colex positions) still open; E <= 496 */
    double proximity, eigenvalue;
    int32_t diameter, k;
    float cost, eval;
    int32_t agent;
    uint32_t node;
} azd_dense_ah_argmin;
int azd_engine_dense_ah_argmin_data(azd_engine *e, azd_dense_ah_argmin *out);
/* ArgminData of an engine with AZD_ENGINE_DENSE_AH_WIDE beside AZD_ENGINE_DENSE_AH (on any other engine: AZD_ERR_UNSUPPORTED) */
typedef struct azd_dense_ah_wide_argmin {
    uint64_t adj[64];
    uint64_t permitted[32]; /* modifiable slots (colex positions) still open; E <= 2016 */
    double proximity, eigenvalue;
    int32_t diameter, k;
    float cost, eval;
    int32_t agent;
    uint32_t node;
} azd_dense_ah_wide_argmin;
int azd_engine_dense_ah_wide_argmin_data(azd_engine *e, azd_dense_ah_wide_argmin *out);
/* the cost of agent `agent`'s current state as the engine keeps it (the AH counterpart of azd_engine_agent_state's lambda_1 /
 * matching_size) */
int azd_engine_dense_ah_agent_cost(azd_engine *e, int agent, azd_dense_ah_cost_t *out);

/* ---- Weighted-invariant cost: the dense-graph space's third objective (AZD_ENGINE_DENSE_INV engines minimise it), BUILD-DEFINED
 * (DESIGN.md "The invariant cost").  Ten invariants of a CONNECTED graph on n vertices, in this order -- index and name are ABI:
 *   0 edges         m                                   5 proximity     min_u t(u) / (n - 1)       (one f64 division)
 *   1 max_degree                                        6 remoteness    max_u t(u) / (n - 1)       (one f64 division)
 *   2 min_degree                                        7 avg_distance  sum_u t(u) / (n (n - 1))   (integer sum, one f64 division)
 *   3 diameter      D = largest eccentricity            8 adj_eig       adjacency eigenvalue at descending index adj_index
 *   4 radius        smallest eccentricity               9 dist_eig      distance-matrix eigenvalue at descending index dist_index,
 *                                                                       or (AZD_DENSE_INV_INDEX_AH) k = 2D/3 - 1, n - 1 when 2D/3 = 0
 * (t(u) = sum_v d(u, v), the transmission), combined by a recipe the caller gives at run time:
 *   c = bias;  for i = 0 .. 9 in order, if weight[i] != 0:  c = c + weight[i] * I_i   (two IEEE f64 operations, never fused)
 *   cost = (float)c;  eval = eval_scale * (cost + eval_offset)                         (f32, this order)
 * A spectral invariant (8, 9) whose weight is zero is not computed: it is reported as 0.0 and its bit of `computed` is clear; the
 * eight others are always computed and reported.  The eigenvalues come from the Aouchiche-Hansen cost's procedure (Householder
 * reduction, Sturm-count multisection), so host function, device kernel and the tests' Python reference agree bit for bit; with
 * weight[5] = weight[9] = 1, bias 0, dist_index = AZD_DENSE_INV_INDEX_AH, eval_offset 2.0f and eval_scale 1.0f / (2n + 2) cost
 * and eval are azd_dense_ah_cost's.  The matching number is not in the list: it needs the default cost's per-node matching arena
 * and repair; lambda_1 + matching number stays the default tier's objective. */
#define AZD_DENSE_INV_MAX_N 32
/* ... of the 64-row form, which has names of its own: azd_dense_inv_cost_wide, AZD_ENGINE_DENSE_INV_WIDE */
#define AZD_DENSE_INV_WIDE_MAX_N 64
#define AZD_DENSE_INV_COUNT 10
#define AZD_DENSE_INV_INDEX_AH (-1)
#define AZD_DENSE_INV_NAMES "edges", "max_degree", "min_degree", "diameter", "radius", "proximity", "remoteness", "avg_distance", "adj_eig", "dist_eig"
typedef struct azd_dense_inv_recipe {
    double weight[AZD_DENSE_INV_COUNT];
    double bias;
    int adj_index;     /* 0 .. n - 1 */
    int dist_index;    /* 0 .. n - 1, or AZD_DENSE_INV_INDEX_AH */
    float eval_offset;
    float eval_scale;  /* not zero */
} azd_dense_inv_recipe;
typedef struct azd_dense_inv_cost_t {
    double inv[AZD_DENSE_INV_COUNT];
    int dist_k;        /* the distance index the recipe resolves to on this graph */
    uint32_t computed; /* bit i: inv[i] was computed (0xFF always; bits 8, 9 by the weights) */
    float cost;
    float eval;
} azd_dense_inv_cost_t;
/* The cost on the host; needs no GPU.  The graph is checked like azd_dense_ah_cost's (4 <= n <= AZD_DENSE_INV_MAX_N, simple,
 * symmetric, connected), the recipe like azd_engine_set_dense_inv_recipe's: AZD_ERR_INVALID_ARGUMENT naming the argument or field. */
int azd_dense_inv_cost(const uint64_t *adj, int n, const azd_dense_inv_recipe *recipe, azd_dense_inv_cost_t *out);
/* The same host function for 4 <= n <= AZD_DENSE_INV_WIDE_MAX_N: the same sequence of IEEE f64 operations, the same graph and
 * recipe checks (the indices against 0 .. n - 1); at n <= 32 the same bytes as azd_dense_inv_cost.  In both, as in
 * azd_dense_invx_cost and on the device, at every n: a Householder step whose column has less than 2^-200 below the subdiagonal
 * (sum of squares) is skipped like one that has nothing there -- the trailing block of a rank-deficient matrix (the adjacency
 * matrix of a complete bipartite graph, of a double broom) is rounding noise that otherwise shrinks into subnormal squares and
 * ends in NaN, from 19 vertices on.  The entries dropped are below 2^-100, far inside the procedure's backward error. */
int azd_dense_inv_cost_wide(const uint64_t *adj, int n, const azd_dense_inv_recipe *recipe, azd_dense_inv_cost_t *out);
/* The device kernel in isolation: the cost of `count` graphs on n vertices (adj[count][n]) under one recipe, one wavefront each,
 * repeated `reps` times; *ms = GPU time of the timed launch.  Graphs and recipe are checked before the device is looked for. */
int azd_debug_probe_inv_cost(int device, const uint64_t *adj, int n, int count, int reps, const azd_dense_inv_recipe *recipe,
                             azd_dense_inv_cost_t *out, float *ms);
/* ... and the 64-row kernel (AZD_ENGINE_DENSE_INV_WIDE engines' cost), 4 <= n <= AZD_DENSE_INV_WIDE_MAX_N; checked the same way */
int azd_debug_probe_inv_cost_wide(int device, const uint64_t *adj, int n, int count, int reps, const azd_dense_inv_recipe *recipe,
                                  azd_dense_inv_cost_t *out, float *ms);
/* The recipe of an AZD_ENGINE_DENSE_INV engine: set once, between azd_engine_create and the first par_new (par_new on such an engine
 * without a recipe is refused and names this call; once par_new has run the recipe is fixed -- a tree's evals must mean one thing --
 * and this call is AZD_ERR_INVALID_ARGUMENT).  AZD_ERR_INVALID_ARGUMENT naming the field: a weight, the bias, eval_offset or
 * eval_scale not finite; eval_scale 0; all ten weights zero; an index outside its range.  AZD_ERR_UNSUPPORTED on an engine of
 * another tier. */
int azd_engine_set_dense_inv_recipe(azd_engine *e, const azd_dense_inv_recipe *recipe);
/* ArgminData of an AZD_ENGINE_DENSE_INV engine: the graph, the slots still open, the cost record */
typedef struct azd_dense_inv_argmin {
    uint64_t adj[32];
    uint64_t permitted[8]; /* modifiable slots (colex positions) still open; E <= 496 */
    double inv[AZD_DENSE_INV_COUNT];
    int32_t dist_k;
    uint32_t computed;
    float cost;
    float eval;
    int32_t agent;
    uint32_t node;
} azd_dense_inv_argmin;
int azd_engine_dense_inv_argmin_data(azd_engine *e, azd_dense_inv_argmin *out);
/* ArgminData of an engine with AZD_ENGINE_DENSE_INV_WIDE beside AZD_ENGINE_DENSE_INV (on any other engine: AZD_ERR_UNSUPPORTED) */
typedef struct azd_dense_inv_wide_argmin {
    uint64_t adj[64];
    uint64_t permitted[32]; /* modifiable slots (colex positions) still open; E <= 2016 */
    double inv[AZD_DENSE_INV_COUNT];
    int32_t dist_k;
    uint32_t computed;
    float cost;
    float eval;
    int32_t agent;
    uint32_t node;
} azd_dense_inv_wide_argmin;
int azd_engine_dense_inv_wide_argmin_data(azd_engine *e, azd_dense_inv_wide_argmin *out);
/* the cost record of agent `agent`'s current state as the engine keeps it (cost and eval recomputed from the kept invariants) */
int azd_engine_dense_inv_agent_cost(azd_engine *e, int agent, azd_dense_inv_cost_t *out);

/* ---- Extended invariant cost (AZD_ENGINE_DENSE_INVX engines minimise it), BUILD-DEFINED (DESIGN.md "The extended invariant
 * cost").  Sixteen invariants of a CONNECTED graph on 4 <= n <= 32 vertices -- index and name are ABI.  0 .. 9 are the
 * weighted-invariant cost's, names and definitions unchanged; then
 *   10 lap_eig    eigenvalue of L = D - A at descending index lap_index (n - 2: the algebraic connectivity)
 *   11 slap_eig   eigenvalue of Q = D + A at descending index slap_index
 *   12 randic     sum over edges uv of 1 / sqrt(d_u d_v)      (f64: per vertex u over its neighbours v < u ascending, one division
 *                                                              and one square root per edge, summed with compensation (TwoSum), then
 *                                                              the cost's balanced tree sum: within n 2^-52 of the exact sum of
 *                                                              the terms on the tests' 560 graphs)
 *   13 zagreb1    sum over vertices of d_u^2                  14 zagreb2    sum over edges uv of d_u d_v
 *   15 triangles  (sum over edges uv of |N(u) & N(v)|) / 3
 * combined by a recipe the caller gives at run time: the linear part as above over sixteen weights, then up to four PAIR TERMS
 *   c = bias;  for i = 0 .. 15 in order, if weight[i] != 0:  c = c + weight[i] * I_i              (two IEEE f64 operations)
 *   for t = 0 .. n_terms - 1 in order, if coef_t != 0:  v = I_a * I_b or I_a / I_b;  c = c + coef_t * v   (three)
 *   cost = (float)c;  eval = eval_scale * (cost + eval_offset)
 * The eight integer invariants 0 .. 7 are always computed.  Each of 8 .. 15 is computed only when its weight is not zero or a pair
 * term with a coefficient that is not zero names it; otherwise it is reported as 0.0 and its bit of `computed` is clear.  The
 * divisor of a DIV term must be an invariant that is positive on every connected graph with n >= 4 -- indices 0 .. 7, 12, 13, 14 --
 * so the cost is always finite.  With weights 10 .. 15 zero and n_terms 0 the sequence of operations is the weighted-invariant
 * cost's: inv[0 .. 9], dist_k, cost and eval are azd_dense_inv_cost's bit for bit. */
#define AZD_DENSE_INVX_MAX_N 32
/* ... of the 64-row form, which has names of its own: azd_dense_invx_cost_wide, AZD_ENGINE_DENSE_INVX_WIDE */
#define AZD_DENSE_INVX_WIDE_MAX_N 64
#define AZD_DENSE_INVX_COUNT 16
#define AZD_DENSE_INVX_MAX_TERMS 4
#define AZD_DENSE_INVX_MUL 0
#define AZD_DENSE_INVX_DIV 1
#define AZD_DENSE_INVX_NAMES AZD_DENSE_INV_NAMES, "lap_eig", "slap_eig", "randic", "zagreb1", "zagreb2", "triangles"
typedef struct azd_dense_invx_term {
    double coef;
    int a, b;          /* 0 .. 15 */
    int op;            /* AZD_DENSE_INVX_MUL: I_a * I_b;  AZD_DENSE_INVX_DIV: I_a / I_b (b among 0 .. 7, 12, 13, 14) */
} azd_dense_invx_term;
typedef struct azd_dense_invx_recipe {
    double weight[AZD_DENSE_INVX_COUNT];
    double bias;
    int adj_index;     /* 0 .. n - 1 */
    int dist_index;    /* 0 .. n - 1, or AZD_DENSE_INV_INDEX_AH */
    int lap_index;     /* 0 .. n - 1 */
    int slap_index;    /* 0 .. n - 1 */
    float eval_offset;
    float eval_scale;  /* not zero */
    azd_dense_invx_term term[AZD_DENSE_INVX_MAX_TERMS];
    int n_terms;       /* 0 .. 4 */
} azd_dense_invx_recipe;
typedef struct azd_dense_invx_cost_t {
    double inv[AZD_DENSE_INVX_COUNT];
    int dist_k;        /* the distance index the recipe resolves to on this graph */
    uint32_t computed; /* bit i: inv[i] was computed (0xFF always; bits 8 .. 15 by the weights and the pair terms) */
    float cost;
    float eval;
} azd_dense_invx_cost_t;
/* The cost on the host; needs no GPU.  The graph is checked like azd_dense_inv_cost's, the recipe like
 * azd_engine_set_dense_invx_recipe's: AZD_ERR_INVALID_ARGUMENT naming the argument or field. */
int azd_dense_invx_cost(const uint64_t *adj, int n, const azd_dense_invx_recipe *recipe, azd_dense_invx_cost_t *out);
/* The same host function for 4 <= n <= AZD_DENSE_INVX_WIDE_MAX_N: the same sequence of IEEE f64 operations, the same graph and
 * recipe checks (the indices against 0 .. n - 1); at n <= 32 the same bytes as azd_dense_invx_cost. */
int azd_dense_invx_cost_wide(const uint64_t *adj, int n, const azd_dense_invx_recipe *recipe, azd_dense_invx_cost_t *out);
/* The device kernel in isolation, as azd_debug_probe_inv_cost: graphs and recipe are checked before the device is looked for. */
int azd_debug_probe_invx_cost(int device, const uint64_t *adj, int n, int count, int reps, const azd_dense_invx_recipe *recipe,
                              azd_dense_invx_cost_t *out, float *ms);
/* ... and the 64-row kernel (AZD_ENGINE_DENSE_INVX_WIDE engines' cost), 4 <= n <= AZD_DENSE_INVX_WIDE_MAX_N; checked the same way */
int azd_debug_probe_invx_cost_wide(int device, const uint64_t *adj, int n, int count, int reps, const azd_dense_invx_recipe *recipe,
                                   azd_dense_invx_cost_t *out, float *ms);
/* The recipe of an AZD_ENGINE_DENSE_INVX engine (with or without AZD_ENGINE_DENSE_INVX_WIDE): set once, between azd_engine_create and the first par_new (par_new without it is
 * refused and names this call; after par_new this call is AZD_ERR_INVALID_ARGUMENT).  AZD_ERR_INVALID_ARGUMENT naming the field:
 * a weight, coefficient, the bias, eval_offset or eval_scale not finite; eval_scale 0; all weights and all coefficients zero;
 * n_terms outside 0 .. 4; a term's a or b outside 0 .. 15, its op unknown, or a divisor outside 0 .. 7, 12, 13, 14; an index
 * outside its range.  AZD_ERR_UNSUPPORTED on an engine of another tier. */
int azd_engine_set_dense_invx_recipe(azd_engine *e, const azd_dense_invx_recipe *recipe);
/* ArgminData of an AZD_ENGINE_DENSE_INVX engine: the graph, the slots still open, the cost record */
typedef struct azd_dense_invx_argmin {
    uint64_t adj[32];
    uint64_t permitted[8]; /* modifiable slots (colex positions) still open; E <= 496 */
    double inv[AZD_DENSE_INVX_COUNT];
    int32_t dist_k;
    uint32_t computed;
    float cost;
    float eval;
    int32_t agent;
    uint32_t node;
} azd_dense_invx_argmin;
int azd_engine_dense_invx_argmin_data(azd_engine *e, azd_dense_invx_argmin *out);
/* ArgminData of an engine with AZD_ENGINE_DENSE_INVX_WIDE beside AZD_ENGINE_DENSE_INVX (on any other engine: AZD_ERR_UNSUPPORTED) */
typedef struct azd_dense_invx_wide_argmin {
    uint64_t adj[64];
    uint64_t permitted[32]; /* modifiable slots (colex positions) still open; E <= 2016 */
    double inv[AZD_DENSE_INVX_COUNT];
    int32_t dist_k;
    uint32_t computed;
    float cost;
    float eval;
    int32_t agent;
    uint32_t node;
} azd_dense_invx_wide_argmin;
int azd_engine_dense_invx_wide_argmin_data(azd_engine *e, azd_dense_invx_wide_argmin *out);
/* the cost record of agent `agent`'s current state as the engine keeps it (cost and eval recomputed from the kept invariants) */
int azd_engine_dense_invx_agent_cost(azd_engine *e, int agent, azd_dense_invx_cost_t *out);

/* ---- Spectrum invariant cost (AZD_ENGINE_DENSE_INVS engines minimise it), BUILD-DEFINED (DESIGN.md "The spectrum invariant
 * cost").  Twenty-one invariants of a CONNECTED graph on 4 <= n <= 32 vertices -- index and name are ABI.  0 .. 15 are the extended
 * invariant cost's, names and definitions unchanged; then, with theta_0 <= .. <= theta_{n-1} ALL eigenvalues of a matrix,
 *   16 adj_energy   sum_l |theta_l(A)|         (the graph energy)
 *   17 dist_energy  sum_l |theta_l(D)|         (D the distance matrix)
 *   18 lap_energy   sum_l |theta_l(L) - s|     (L = Deg - A;  s = (double)(sum of degrees) / (double)n, the mean degree)
 *   19 slap_energy  sum_l |theta_l(Q) - s|     (Q = Deg + A)
 *   20 adj_spread   theta_{n-1}(A) - theta_0(A)
 * Whole-spectrum procedure (one definition for device, host and the tests' reference; every f64 step one IEEE operation): on the
 * tridiagonal form that the matrix's reduction leaves -- the same Householder steps and deflation rule as for the one eigenvalue
 * by index -- with R the Gershgorin bound, eigenvalue l starts from hi = R + 1, lo = -hi and makes AZD_DENSE_INVS_ROUNDS = 67
 * rounds of x = (lo + hi) * 0.5, c = the Sturm count at x, `c <= l ? lo = x : hi = x`; theta_l = (lo + hi) * 0.5.  The final
 * bracket 2 (R + 1) 2^-67 is no wider than the one-eigenvalue multisection's 2 (R + 1) 65^-11.  An energy is the balanced tree
 * sum over 64 slots (slots >= n hold 0.0).
 * A matrix is reduced at most once per cost; then the multisection runs only when its *_eig is needed and the whole-spectrum
 * procedure only when its energy (or, for A, the spread) is.  Needed, as in the extended cost: a weight that is not zero, or a pair
 * term with a coefficient that is not zero that names it; otherwise the invariant is reported as 0.0 and its bit of `computed`
 * (8 .. 20) is clear.  The combination rule is the extended cost's over twenty-one weights.  A DIV term's divisor is one of 0 .. 7,
 * 12, 13, 14, 16 .. 20: all five new invariants are positive on every connected graph with n >= 4.  With weights 16 .. 20 zero and
 * no term naming 16 .. 20 the sequence of operations is the extended invariant cost's: inv[0 .. 15], dist_k, computed, cost and
 * eval are azd_dense_invx_cost's bit for bit. */
#define AZD_DENSE_INVS_MAX_N 32
/* ... of the 64-row form, which has names of its own: azd_dense_invs_cost_wide, AZD_ENGINE_DENSE_INVS_WIDE */
#define AZD_DENSE_INVS_WIDE_MAX_N 64
#define AZD_DENSE_INVS_COUNT 21
#define AZD_DENSE_INVS_ROUNDS 67
#define AZD_DENSE_INVS_NAMES AZD_DENSE_INVX_NAMES, "adj_energy", "dist_energy", "lap_energy", "slap_energy", "adj_spread"
/* the matrices azd_dense_invs_spectrum knows */
#define AZD_DENSE_INVS_MATRIX_ADJ 0
#define AZD_DENSE_INVS_MATRIX_DIST 1
#define AZD_DENSE_INVS_MATRIX_LAP 2
#define AZD_DENSE_INVS_MATRIX_SLAP 3
typedef struct azd_dense_invs_recipe {
    double weight[AZD_DENSE_INVS_COUNT];
    double bias;
    int adj_index;     /* 0 .. n - 1 */
    int dist_index;    /* 0 .. n - 1, or AZD_DENSE_INV_INDEX_AH */
    int lap_index;     /* 0 .. n - 1 */
    int slap_index;    /* 0 .. n - 1 */
    float eval_offset;
    float eval_scale;  /* not zero */
    azd_dense_invx_term term[AZD_DENSE_INVX_MAX_TERMS]; /* a, b in 0 .. 20; a divisor b among 0 .. 7, 12, 13, 14, 16 .. 20 */
    int n_terms;       /* 0 .. 4 */
} azd_dense_invs_recipe;
typedef struct azd_dense_invs_cost_t {
    double inv[AZD_DENSE_INVS_COUNT];
    int dist_k;        /* the distance index the recipe resolves to on this graph */
    uint32_t computed; /* bit i: inv[i] was computed (0xFF always; bits 8 .. 20 by the weights and the pair terms) */
    float cost;
    float eval;
} azd_dense_invs_cost_t;
/* The cost on the host; needs no GPU.  The graph is checked like azd_dense_invx_cost's, the recipe like
 * azd_engine_set_dense_invs_recipe's: AZD_ERR_INVALID_ARGUMENT naming the argument or field. */
int azd_dense_invs_cost(const uint64_t *adj, int n, const azd_dense_invs_recipe *recipe, azd_dense_invs_cost_t *out);
/* The same host function for 4 <= n <= AZD_DENSE_INVS_WIDE_MAX_N: the same sequence of IEEE f64 operations, the same graph and
 * recipe checks (the indices against 0 .. n - 1); at n <= 32 the same bytes as azd_dense_invs_cost. */
int azd_dense_invs_cost_wide(const uint64_t *adj, int n, const azd_dense_invs_recipe *recipe, azd_dense_invs_cost_t *out);
/* Host only: theta_0 <= .. <= theta_{n-1} of matrix `which` (AZD_DENSE_INVS_MATRIX_*) by the whole-spectrum procedure, n doubles
 * -- what the energies and the spread are summed from, so that each eigenvalue can be checked.  The graph is checked as above. */
int azd_dense_invs_spectrum(const uint64_t *adj, int n, int which, double *out);
/* ... for 4 <= n <= AZD_DENSE_INVS_WIDE_MAX_N; at n <= 32 the same bytes */
int azd_dense_invs_spectrum_wide(const uint64_t *adj, int n, int which, double *out);
/* The device kernel in isolation, as azd_debug_probe_invx_cost: graphs and recipe are checked before the device is looked for. */
int azd_debug_probe_invs_cost(int device, const uint64_t *adj, int n, int count, int reps, const azd_dense_invs_recipe *recipe,
                              azd_dense_invs_cost_t *out, float *ms);
/* ... and the 64-row kernel (AZD_ENGINE_DENSE_INVS_WIDE engines' cost), 4 <= n <= AZD_DENSE_INVS_WIDE_MAX_N; checked the same way */
int azd_debug_probe_invs_cost_wide(int device, const uint64_t *adj, int n, int count, int reps, const azd_dense_invs_recipe *recipe,
                                   azd_dense_invs_cost_t *out, float *ms);
/* The recipe of an AZD_ENGINE_DENSE_INVS engine (with or without AZD_ENGINE_DENSE_INVS_WIDE): set once, between azd_engine_create and the first par_new (par_new without it is
 * refused and names this call; after par_new this call is AZD_ERR_INVALID_ARGUMENT).  AZD_ERR_INVALID_ARGUMENT naming the field,
 * as azd_engine_set_dense_invx_recipe, with a term's a or b in 0 .. 20.  AZD_ERR_UNSUPPORTED on an engine of another tier. */
int azd_engine_set_dense_invs_recipe(azd_engine *e, const azd_dense_invs_recipe *recipe);
/* ArgminData of an AZD_ENGINE_DENSE_INVS engine: the graph, the slots still open, the cost record */
typedef struct azd_dense_invs_argmin {
    uint64_t adj[32];
    uint64_t permitted[8]; /* modifiable slots (colex positions) still open; E <= 496 */
    double inv[AZD_DENSE_INVS_COUNT];
    int32_t dist_k;
    uint32_t computed;
    float cost;
    float eval;
    int32_t agent;
    uint32_t node;
} azd_dense_invs_argmin;
int azd_engine_dense_invs_argmin_data(azd_engine *e, azd_dense_invs_argmin *out);
/* ArgminData of an engine with AZD_ENGINE_DENSE_INVS_WIDE beside AZD_ENGINE_DENSE_INVS (on any other engine: AZD_ERR_UNSUPPORTED) */
typedef struct azd_dense_invs_wide_argmin {
    uint64_t adj[64];
    uint64_t permitted[32]; /* modifiable slots (colex positions) still open; E <= 2016 */
    double inv[AZD_DENSE_INVS_COUNT];
    int32_t dist_k;
    uint32_t computed;
    float cost;
    float eval;
    int32_t agent;
    uint32_t node;
} azd_dense_invs_wide_argmin;
int azd_engine_dense_invs_wide_argmin_data(azd_engine *e, azd_dense_invs_wide_argmin *out);
/* the cost record of agent `agent`'s current state as the engine keeps it (cost and eval recomputed from the kept invariants) */
int azd_engine_dense_invs_agent_cost(azd_engine *e, int agent, azd_dense_invs_cost_t *out);
/* Parity probe for the f64 primitives the AH cost depends on bit for bit.  in: 2*n doubles (pairs x, y); out: 3*n doubles per
 * pair: [0] x / y, [1] sqrt(|x|), [2] x - (x / y) * y (two roundings: a contracted form would differ). */
int azd_debug_probe_math_f64(int device, const double *in, double *out, int n);

/* The evaluator's bf16 forward GEMM in isolation (timing, tests): Y[M, N] = act(A[M, K] . W[N, K]^T + bias) on device
 * pointers; A and W are bf16 rows of pitch Kp (a multiple of 64, zero beyond K), Y f32 or bf16 with pitch ldy;
 * *ms = mean GPU time of `reps` launches. */
int azd_debug_gemm_bf16(int device, int M, int N, int Kp, const void *d_a, const void *d_w, const float *d_bias, void *d_y, int ldy,
                        int out_bf16, int act, int reps, float *ms);

#ifdef __cplusplus
}
#endif
#endif /* AZDOPT_AMD_H */
