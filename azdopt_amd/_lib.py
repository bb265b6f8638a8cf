"""ctypes loader of libazdopt_amd.so (the C ABI declared in include/azdopt_amd.h).

There is no Python or CPU fallback: if the HIP library is missing or no gfx950
device is visible, the product fails loudly."""
import ctypes as C
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("AZD_LIB", os.path.join(_HERE, "libazdopt_amd.so"))
_LIB = None

CTR = dict(EXPANSIONS=0, TERMINALS=1, TRANSPOSITIONS=2, VISITED_STEPS=3, SELECT_CALLS=4, SUM_DEG=5,
           SUM_ACTIONS=6, CASCADE_NODES=7, NEW_PREDS=8, ROOT_EXHAUSTED=9, MAX_FRONTIER=10, MAX_DEPTH=11,
           CURIOSITY_PAIRS=12, EVAL_LAYER_CLOCKS=13, TICKS_ADD_ACTIONS=14, FAILED=15, TICKS_TOTAL=16, TICKS_SELECT=17, TICKS_LOOKUP=18, TICKS_NEWNODE=19,
           TICKS_CASCADE=20, TICKS_MAX_CALL=21, TICKS_LAMBDA=22, TICKS_MATCHING=23, TICKS_WAIT=24, EVAL_BATCHES=25, EVAL_ROWS=26, EVAL_TILES=27, TICKS_TILES=28, TICKS_BATCH=29, TICKS_TILE_SETUP=30, TICKS_TILE_KLOOP=31)
CTR_COUNT = 32

ACT_NONE, ACT_RELU, ACT_SIGMOID = 0, 1, 2
ENGINE_NO_PERSISTENT_STEP = 1
ENGINE_ASYNC_STEP = 2
ENGINE_BARRIER_STEP = 4
ENGINE_POOL_STEP = 8
ENGINE_DENSE_AH = 32    # AZD_ENGINE_DENSE_AH: the dense-graph space with the Aouchiche-Hansen cost (n <= 32)
ENGINE_RAMSEY_U64 = 16  # AZD_ENGINE_RAMSEY_U64: the 64-bit Ramsey tier (n <= 64, E*C <= 2304), beside max_slots > 0
ENGINE_EXT_POOL_STEP = 64  # AZD_ENGINE_EXT_POOL_STEP: Ramsey engines with max_slots > 0: searcher-only pool step, batched GEMMs beside it
ENGINE_DENSE_AH_WIDE = 256  # AZD_ENGINE_DENSE_AH_WIDE: beside ENGINE_DENSE_AH only: the Aouchiche-Hansen cost up to n = 64 (64-row kernels)
ENGINE_EXT_POOL_F32 = 128  # AZD_ENGINE_EXT_POOL_F32: beside ENGINE_EXT_POOL_STEP (Ramsey), alone on SPACE_DENSE: that form with an fp32 model (gathered fp32 GEMMs)
ENGINE_DENSE_INV = 1024  # AZD_ENGINE_DENSE_INV: the dense-graph space with the weighted-invariant cost (n <= 32; recipe set at run time)
ENGINE_DENSE_INV_WIDE = 2048  # AZD_ENGINE_DENSE_INV_WIDE: beside ENGINE_DENSE_INV only: the weighted-invariant cost up to n = 64 (64-row kernels)
ENGINE_DENSE_INVX_WIDE = 8192  # AZD_ENGINE_DENSE_INVX_WIDE: beside ENGINE_DENSE_INVX only: the extended invariant cost up to n = 64 (64-row kernels)
ENGINE_DENSE_INVS_WIDE = 32768  # AZD_ENGINE_DENSE_INVS_WIDE: beside ENGINE_DENSE_INVS only: the spectrum invariant cost up to n = 64 (64-row kernels)
ENGINE_DENSE_INVS = 16384  # AZD_ENGINE_DENSE_INVS: the dense-graph space with the spectrum invariant cost (n <= 32; twenty-one invariants: energies, spread)
ENGINE_DENSE_INVX = 4096  # AZD_ENGINE_DENSE_INVX: the dense-graph space with the extended invariant cost (n <= 32; sixteen invariants, pair terms)
ENGINE_RAMSEY_BIG_CLIQUES = 512  # AZD_ENGINE_RAMSEY_BIG_CLIQUES: beside ENGINE_RAMSEY_U64 only: clique sizes up to 8 (kernels of their own)
SPACE_C21 = 1
SPACE_RAMSEY = 2
SPACE_DENSE = 3
RAMSEY_MAX_N = 23       # AZD_RAMSEY_MAX_N
RAMSEY_WIDE_MAX_N = 32  # AZD_RAMSEY_WIDE_MAX_N: a wide Ramsey engine (EngineConfig.max_slots > 0)
RAMSEY_U64_MAX_N = 64   # AZD_RAMSEY_U64_MAX_N: the 64-bit tier (ENGINE_RAMSEY_U64)
RAMSEY_U64_NODE_ACTIONS = 512  # AZD_RAMSEY_U64_NODE_ACTIONS: max_slots * (C - 1) of the 64-bit tier
RAMSEY_BIG_CLIQUE_MAX = 8  # AZD_RAMSEY_BIG_CLIQUE_MAX: the largest forbidden clique under ENGINE_RAMSEY_BIG_CLIQUES (else 5)
RAMSEY_U64_MAX_ACTIONS = 2304  # E*C of the 64-bit tier (keys of 36 words)
DENSE_AH_MAX_N = 32     # AZD_DENSE_AH_MAX_N: the Aouchiche-Hansen cost (azd_dense_ah_cost)
DENSE_AH_WIDE_MAX_N = 64  # AZD_DENSE_AH_WIDE_MAX_N: its 64-row form (azd_dense_ah_cost_wide, ENGINE_DENSE_AH_WIDE)
DENSE_INV_MAX_N = 32    # AZD_DENSE_INV_MAX_N: the weighted-invariant cost (azd_dense_inv_cost)
DENSE_INV_WIDE_MAX_N = 64  # AZD_DENSE_INV_WIDE_MAX_N: its 64-row form (azd_dense_inv_cost_wide, ENGINE_DENSE_INV_WIDE)
DENSE_INV_COUNT = 10    # AZD_DENSE_INV_COUNT
DENSE_INV_INDEX_AH = -1  # AZD_DENSE_INV_INDEX_AH: dist_index by the Aouchiche-Hansen rule, k = 2D/3 - 1 (n - 1 when 2D/3 = 0)
# AZD_DENSE_INV_NAMES: index and name are ABI
DENSE_INV_NAMES = ("edges", "max_degree", "min_degree", "diameter", "radius", "proximity", "remoteness", "avg_distance", "adj_eig", "dist_eig")
DENSE_INVX_MAX_N = 32   # AZD_DENSE_INVX_MAX_N: the extended invariant cost (azd_dense_invx_cost)
DENSE_INVX_WIDE_MAX_N = 64  # AZD_DENSE_INVX_WIDE_MAX_N: its 64-row form (azd_dense_invx_cost_wide, ENGINE_DENSE_INVX_WIDE)
DENSE_INVX_COUNT = 16   # AZD_DENSE_INVX_COUNT
DENSE_INVX_MAX_TERMS = 4  # AZD_DENSE_INVX_MAX_TERMS: pair terms of a recipe
DENSE_INVX_MUL, DENSE_INVX_DIV = 0, 1  # AZD_DENSE_INVX_MUL / _DIV: a pair term's op
# AZD_DENSE_INVX_NAMES: index and name are ABI; the first ten are DENSE_INV_NAMES
DENSE_INVX_NAMES = DENSE_INV_NAMES + ("lap_eig", "slap_eig", "randic", "zagreb1", "zagreb2", "triangles")
DENSE_INVS_MAX_N = 32   # AZD_DENSE_INVS_MAX_N: the spectrum invariant cost (azd_dense_invs_cost)
DENSE_INVS_WIDE_MAX_N = 64  # AZD_DENSE_INVS_WIDE_MAX_N: its 64-row form (azd_dense_invs_cost_wide, ENGINE_DENSE_INVS_WIDE)
DENSE_INVS_COUNT = 21   # AZD_DENSE_INVS_COUNT
DENSE_INVS_ROUNDS = 67  # AZD_DENSE_INVS_ROUNDS: bisection rounds of the whole-spectrum procedure
# AZD_DENSE_INVS_NAMES: index and name are ABI; the first sixteen are DENSE_INVX_NAMES
DENSE_INVS_NAMES = DENSE_INVX_NAMES + ("adj_energy", "dist_energy", "lap_energy", "slap_energy", "adj_spread")
PATH_SET, PATH_SEQUENCE = 0, 1
ROOT_RULE_THRESHOLD, ROOT_RULE_BEST = 0, 1  # AZD_ROOT_RULE_*
ROOT_RULES = {"threshold": ROOT_RULE_THRESHOLD, "best": ROOT_RULE_BEST}


class AzdError(RuntimeError):
    def __init__(self, status, where):
        L = lib()
        msg = L.azd_status_string(status).decode()
        detail = L.azd_last_error().decode()
        super().__init__(f"{where}: {msg} (status {status}){': ' + detail if detail else ''}")
        self.status = status


class AdamConfig(C.Structure):  # dfdx AdamConfig as set at 04-c21-tree.rs:87-92
    _fields_ = [("lr", C.c_float), ("beta1", C.c_float), ("beta2", C.c_float), ("eps", C.c_float), ("l2", C.c_float)]


class EngineConfig(C.Structure):
    _fields_ = [("space_id", C.c_int), ("n", C.c_int), ("batch", C.c_int), ("device", C.c_int),
                ("node_capacity", C.c_int), ("arc_capacity", C.c_int), ("prediction_capacity", C.c_int),
                ("first_agent", C.c_uint64), ("flags", C.c_uint32),
                ("n_colors", C.c_int), ("clique_sizes", C.c_int * 4), ("color_weights", C.c_float * 4),
                ("path_kind", C.c_int), ("layers", C.c_int), ("max_slots", C.c_int), ("dense_p", C.c_float)]


class RootPolicy(C.Structure):  # azd_root_policy
    _fields_ = [("rule", C.c_int), ("n_color_weights", C.c_int), ("color_weights", C.c_double * 4)]


class RamseyArgmin(C.Structure):  # ArgminData<RamseyCountsNoRecolor, TotalCounts<C>>
    _fields_ = [("colors", C.c_uint8 * 256), ("permitted", C.c_uint64 * 4), ("totals", C.c_int32 * 4),
                ("eval", C.c_float), ("agent", C.c_int32), ("node", C.c_uint32)]


class RamseyWideArgmin(C.Structure):  # the same for any Ramsey engine, wide ones included (E <= 496)
    _fields_ = [("colors", C.c_uint8 * 496), ("permitted", C.c_uint64 * 8), ("totals", C.c_int32 * 4),
                ("eval", C.c_float), ("agent", C.c_int32), ("node", C.c_uint32)]


class DenseArgmin(C.Structure):  # ArgminData of the dense-graph space
    _fields_ = [("adj", C.c_uint64 * 64), ("permitted", C.c_uint64 * 40), ("lambda_1", C.c_double),
                ("matching_size", C.c_int32), ("eval", C.c_float), ("agent", C.c_int32), ("node", C.c_uint32)]


class DenseAhCost(C.Structure):  # azd_dense_ah_cost_t: the Aouchiche-Hansen cost of one connected graph
    _fields_ = [("proximity", C.c_double), ("eigenvalue", C.c_double), ("diameter", C.c_int32), ("k", C.c_int32),
                ("cost", C.c_float), ("eval", C.c_float)]


class DenseAhArgmin(C.Structure):  # azd_dense_ah_argmin: ArgminData of a dense engine with the Aouchiche-Hansen cost
    _fields_ = [("adj", C.c_uint64 * 32), ("permitted", C.c_uint64 * 8), ("proximity", C.c_double), ("eigenvalue", C.c_double),
                ("diameter", C.c_int32), ("k", C.c_int32), ("cost", C.c_float), ("eval", C.c_float), ("agent", C.c_int32),
                ("node", C.c_uint32)]


class DenseInvRecipe(C.Structure):  # azd_dense_inv_recipe: weights of the ten invariants, bias, spectral indices, the eval's offset and scale
    _fields_ = [("weight", C.c_double * 10), ("bias", C.c_double), ("adj_index", C.c_int), ("dist_index", C.c_int),
                ("eval_offset", C.c_float), ("eval_scale", C.c_float)]


class DenseInvCost(C.Structure):  # azd_dense_inv_cost_t
    _fields_ = [("inv", C.c_double * 10), ("dist_k", C.c_int), ("computed", C.c_uint32), ("cost", C.c_float), ("eval", C.c_float)]


class DenseInvArgmin(C.Structure):  # azd_dense_inv_argmin: ArgminData of a dense engine with the weighted-invariant cost
    _fields_ = [("adj", C.c_uint64 * 32), ("permitted", C.c_uint64 * 8), ("inv", C.c_double * 10), ("dist_k", C.c_int32),
                ("computed", C.c_uint32), ("cost", C.c_float), ("eval", C.c_float), ("agent", C.c_int32), ("node", C.c_uint32)]


class DenseInvWideArgmin(C.Structure):  # azd_dense_inv_wide_argmin: the same of an engine with ENGINE_DENSE_INV_WIDE (n <= 64, E <= 2016)
    _fields_ = [("adj", C.c_uint64 * 64), ("permitted", C.c_uint64 * 32), ("inv", C.c_double * 10), ("dist_k", C.c_int32),
                ("computed", C.c_uint32), ("cost", C.c_float), ("eval", C.c_float), ("agent", C.c_int32), ("node", C.c_uint32)]


class DenseInvxTerm(C.Structure):  # azd_dense_invx_term: coef * (I_a * I_b) or coef * (I_a / I_b)
    _fields_ = [("coef", C.c_double), ("a", C.c_int), ("b", C.c_int), ("op", C.c_int)]


class DenseInvxRecipe(C.Structure):  # azd_dense_invx_recipe: sixteen weights, bias, four spectral indices, the eval's offset and scale, pair terms
    _fields_ = [("weight", C.c_double * 16), ("bias", C.c_double), ("adj_index", C.c_int), ("dist_index", C.c_int), ("lap_index", C.c_int),
                ("slap_index", C.c_int), ("eval_offset", C.c_float), ("eval_scale", C.c_float), ("term", DenseInvxTerm * 4), ("n_terms", C.c_int)]


class DenseInvxCost(C.Structure):  # azd_dense_invx_cost_t
    _fields_ = [("inv", C.c_double * 16), ("dist_k", C.c_int), ("computed", C.c_uint32), ("cost", C.c_float), ("eval", C.c_float)]


class DenseInvxArgmin(C.Structure):  # azd_dense_invx_argmin: ArgminData of a dense engine with the extended invariant cost
    _fields_ = [("adj", C.c_uint64 * 32), ("permitted", C.c_uint64 * 8), ("inv", C.c_double * 16), ("dist_k", C.c_int32),
                ("computed", C.c_uint32), ("cost", C.c_float), ("eval", C.c_float), ("agent", C.c_int32), ("node", C.c_uint32)]


class DenseInvsRecipe(C.Structure):  # azd_dense_invs_recipe: twenty-one weights, bias, four spectral indices, the eval's offset and scale, pair terms
    _fields_ = [("weight", C.c_double * 21), ("bias", C.c_double), ("adj_index", C.c_int), ("dist_index", C.c_int), ("lap_index", C.c_int),
                ("slap_index", C.c_int), ("eval_offset", C.c_float), ("eval_scale", C.c_float), ("term", DenseInvxTerm * 4), ("n_terms", C.c_int)]


class DenseInvsCost(C.Structure):  # azd_dense_invs_cost_t
    _fields_ = [("inv", C.c_double * 21), ("dist_k", C.c_int), ("computed", C.c_uint32), ("cost", C.c_float), ("eval", C.c_float)]


class DenseInvsArgmin(C.Structure):  # azd_dense_invs_argmin: ArgminData of a dense engine with the spectrum invariant cost
    _fields_ = [("adj", C.c_uint64 * 32), ("permitted", C.c_uint64 * 8), ("inv", C.c_double * 21), ("dist_k", C.c_int32),
                ("computed", C.c_uint32), ("cost", C.c_float), ("eval", C.c_float), ("agent", C.c_int32), ("node", C.c_uint32)]


class DenseInvsWideArgmin(C.Structure):  # azd_dense_invs_wide_argmin: the same of an engine with ENGINE_DENSE_INVS_WIDE (n <= 64, E <= 2016)
    _fields_ = [("adj", C.c_uint64 * 64), ("permitted", C.c_uint64 * 32), ("inv", C.c_double * 21), ("dist_k", C.c_int32),
                ("computed", C.c_uint32), ("cost", C.c_float), ("eval", C.c_float), ("agent", C.c_int32), ("node", C.c_uint32)]


class DenseInvxWideArgmin(C.Structure):  # azd_dense_invx_wide_argmin: the same of an engine with ENGINE_DENSE_INVX_WIDE (n <= 64, E <= 2016)
    _fields_ = [("adj", C.c_uint64 * 64), ("permitted", C.c_uint64 * 32), ("inv", C.c_double * 16), ("dist_k", C.c_int32),
                ("computed", C.c_uint32), ("cost", C.c_float), ("eval", C.c_float), ("agent", C.c_int32), ("node", C.c_uint32)]


class DenseAhWideArgmin(C.Structure):  # azd_dense_ah_wide_argmin: the same of an engine with ENGINE_DENSE_AH_WIDE (n <= 64, E <= 2016)
    _fields_ = [("adj", C.c_uint64 * 64), ("permitted", C.c_uint64 * 32), ("proximity", C.c_double), ("eigenvalue", C.c_double),
                ("diameter", C.c_int32), ("k", C.c_int32), ("cost", C.c_float), ("eval", C.c_float), ("agent", C.c_int32),
                ("node", C.c_uint32)]


class Argmin(C.Structure):  # ArgminData<State, Cost>, az-discrete-opt/src/log.rs:1-11
    _fields_ = [("parents", C.c_uint8 * 32), ("permitted", C.c_uint64 * 4), ("lambda_1", C.c_double),
                ("matching_size", C.c_int32), ("matching", C.c_int32 * 32), ("eval", C.c_float),
                ("agent", C.c_int32), ("node", C.c_uint32)]


def build(force=False):
    """Compile the HIP library for gfx950 (cross-compiles without a GPU)."""
    if force or not os.path.exists(LIB_PATH):
        subprocess.check_call(["make", "-s", "-j4", "-C", os.path.join(_HERE, "csrc")])
    else:
        subprocess.check_call(["make", "-s", "-j4", "-C", os.path.join(_HERE, "csrc")])
    return LIB_PATH


def lib():
    global _LIB
    if _LIB is not None:
        return _LIB
    if not os.path.exists(LIB_PATH):
        raise ImportError(f"{LIB_PATH} is missing: run __graft_entry__.build() (hipcc --offload-arch=gfx950); "
                          "azdopt_amd has no CPU fallback")
    L = C.CDLL(LIB_PATH)
    vp, i32p, u64p, f32p = C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_uint64), C.POINTER(C.c_float)

    def sig(name, res, *args):
        f = getattr(L, name, None)
        if f is None:
            if "AZD_LIB" in os.environ:  # an older / experiment build selected by hand may lack the newer entry points
                return
            raise AttributeError("%s does not export %s" % (LIB_PATH, name))
        f.restype = res
        f.argtypes = list(args)

    sig("azd_status_string", C.c_char_p, C.c_int)
    sig("azd_last_error", C.c_char_p)
    sig("azd_version", C.c_int)
    sig("azd_device_count", C.c_int)
    sig("azd_c21_state_dim", C.c_int, C.c_int)
    sig("azd_c21_action_dim", C.c_int, C.c_int)
    sig("azd_c21_key_words", C.c_int, C.c_int)
    sig("azd_c21_generate_roots", C.c_int, C.c_uint64, C.c_uint64, C.c_uint64, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp)
    sig("azd_evaluator_create_mlp", C.c_int, C.POINTER(vp), C.c_int, C.c_int, C.c_int, C.c_int, vp, C.c_int, C.c_int,
        C.POINTER(AdamConfig), C.c_uint64)
    sig("azd_evaluator_create_trivial", C.c_int, C.POINTER(vp), C.c_int, C.c_int, C.c_int)
    sig("azd_evaluator_create_hash_stream", C.c_int, C.POINTER(vp), C.c_int, C.c_int, C.c_int, C.c_uint64, C.c_uint64)
    sig("azd_evaluator_destroy", C.c_int, vp)
    sig("azd_evaluator_write_predictions", C.c_int, vp, C.c_int, vp, vp)
    sig("azd_evaluator_update_model", C.c_int, vp, C.c_int, vp, vp, vp, f32p)
    sig("azd_evaluator_write_predictions_dev", C.c_int, vp, C.c_int, vp, vp, vp)
    sig("azd_evaluator_update_model_dev", C.c_int, vp, C.c_int, vp, vp, vp, f32p, vp)
    sig("azd_evaluator_set_weight_storage", C.c_int, vp, C.c_int)
    sig("azd_evaluator_num_params", C.c_int64, vp)
    sig("azd_evaluator_get_params", C.c_int, vp, vp)
    sig("azd_evaluator_set_params", C.c_int, vp, vp)
    sig("azd_evaluator_calls", C.c_uint64, vp)
    sig("azd_engine_create", C.c_int, C.POINTER(vp), C.POINTER(EngineConfig), vp)
    sig("azd_engine_destroy", C.c_int, vp)
    sig("azd_engine_par_new", C.c_int, vp, vp, vp)
    sig("azd_engine_par_roll_out_episodes", C.c_int, vp, vp, C.c_int, C.c_uint32, C.c_int, i32p)
    sig("azd_engine_run_ahead", C.c_int, vp, vp, C.c_int, C.c_uint32, C.c_int, i32p)
    sig("azd_engine_par_update_model", C.c_int, vp, C.c_uint32, f32p)
    sig("azd_engine_par_update_model_sharded", C.c_int, vp, C.c_uint32, vp, f32p)
    sig("azd_engine_par_reset_trees", C.c_int, vp, vp, vp)
    sig("azd_engine_argmin_data", C.c_int, vp, C.POINTER(Argmin))
    sig("azd_engine_agent_counters", C.c_int, vp, vp)
    sig("azd_engine_agent_counters_per_agent", C.c_int, vp)
    sig("azd_engine_pool_agent_finish", C.c_int, vp, vp)
    sig("azd_engine_pool_groups", C.c_int, vp, vp, vp, vp)
    sig("azd_engine_ramsey_argmin_data", C.c_int, vp, C.POINTER(RamseyArgmin))
    sig("azd_engine_ramsey_wide_argmin_data", C.c_int, vp, C.POINTER(RamseyWideArgmin))
    sig("azd_engine_ramsey_argmin_any", C.c_int, vp, vp, C.c_int, vp, C.c_int, vp, f32p, i32p, C.POINTER(C.c_uint32))
    sig("azd_engine_ramsey_agent_counts", C.c_int, vp, C.c_int, vp, vp)
    sig("azd_ramsey_state_dim", C.c_int, C.c_int, C.c_int)
    sig("azd_ramsey_action_dim", C.c_int, C.c_int, C.c_int)
    sig("azd_ramsey_key_words", C.c_int, C.c_int, C.c_int)
    sig("azd_ramsey_generate_roots", C.c_int, C.c_uint64, C.c_uint64, C.c_uint64, C.c_int, C.c_int, C.c_int, C.c_int,
        C.c_int, vp, vp)
    sig("azd_ramsey_generate_roots_weighted", C.c_int, C.c_uint64, C.c_uint64, C.c_uint64, C.c_int, C.c_int, C.c_int, C.c_int,
        C.c_int, vp, vp, vp)
    sig("azd_engine_set_root_policy", C.c_int, vp, C.POINTER(RootPolicy))
    sig("azd_engine_get_root_policy", C.c_int, vp, C.POINTER(RootPolicy))
    sig("azd_root_policy_check", C.c_int, C.c_int, C.c_int, C.POINTER(RootPolicy))
    sig("azd_engine_root_policy_report", C.c_int, vp, vp, vp, vp)
    sig("azd_dense_state_dim", C.c_int, C.c_int)
    sig("azd_dense_action_dim", C.c_int, C.c_int)
    sig("azd_dense_key_words", C.c_int, C.c_int)
    sig("azd_dense_generate_roots", C.c_int, C.c_uint64, C.c_uint64, C.c_uint64, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, vp, vp)
    sig("azd_engine_dense_argmin_data", C.c_int, vp, C.POINTER(DenseArgmin))
    sig("azd_c21_modify_roots", C.c_int, vp, C.c_uint64, C.c_uint64, C.c_int, C.c_int, vp, vp)
    sig("azd_c21_modify_roots_dev", C.c_int, vp, C.c_uint64, C.c_uint64, C.c_int, C.c_int, vp, vp)
    sig("azd_engine_par_reset_trees_c21", C.c_int, vp, C.c_uint64, C.c_uint64, C.c_int, C.c_int)
    sig("azd_engine_modify_roots_dev", C.c_int, vp, C.c_uint64, C.c_uint64, C.c_int, C.c_int, vp, vp)
    sig("azd_engine_par_reset_trees_policy", C.c_int, vp, C.c_uint64, C.c_uint64, C.c_int, C.c_int)
    sig("azd_engine_par_new_begin", C.c_int, vp, vp, vp)
    sig("azd_engine_par_new_end", C.c_int, vp, vp)
    sig("azd_engine_roll_out_begin", C.c_int, vp, vp, C.c_int, C.c_uint32)
    sig("azd_engine_roll_out_end", C.c_int, vp, vp, i32p)
    sig("azd_engine_reset_begin", C.c_int, vp, vp, vp)
    sig("azd_engine_reset_end", C.c_int, vp, vp)
    sig("azd_engine_observe", C.c_int, vp, C.c_uint32, vp, vp, vp)
    sig("azd_engine_observe_dev", C.c_int, vp, C.c_uint32, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp))
    sig("azd_engine_read_state_vecs", C.c_int, vp, vp)
    sig("azd_engine_read_predictions", C.c_int, vp, vp)
    sig("azd_engine_debug_tile_forward", C.c_int, vp, vp, vp, C.c_int)
    sig("azd_engine_tree_sizes", C.c_int, vp, C.c_int, i32p, i32p, i32p)
    sig("azd_engine_export_tree", C.c_int, vp, C.c_int, *([vp] * 13))
    sig("azd_engine_agent_state", C.c_int, vp, C.c_int, vp, vp, vp, C.POINTER(C.c_uint32), C.POINTER(C.c_double), i32p)
    sig("azd_engine_counters", C.c_int, vp, vp)
    sig("azd_engine_set_timing", C.c_int, vp, C.c_int)
    sig("azd_engine_timing", C.c_int, vp, C.POINTER(C.c_double), C.POINTER(C.c_double), u64p)
    sig("azd_engine_stream", vp, vp)
    sig("azd_engine_step_form", C.c_int, vp, i32p, C.POINTER(C.c_char_p))
    sig("azd_engine_pool_split", C.c_int, vp, i32p, i32p)
    sig("azd_engine_pool_utilisation", C.c_int, vp, C.POINTER(C.c_double), C.POINTER(C.c_double))
    sig("azd_debug_probe_xcc", C.c_int, C.c_int, vp, C.c_int)
    sig("azd_debug_hash_stream_via_evaluators", C.c_int, vp, C.c_int)
    sig("azd_debug_ext_pool_plan", C.c_int, C.POINTER(EngineConfig), i32p, C.POINTER(C.c_size_t))
    sig("azd_debug_mlp_gradients", C.c_int, vp, C.c_int, vp, vp, vp, vp, f32p)
    sig("azd_debug_write_predictions_gathered", C.c_int, vp, C.c_int, vp, C.c_int, vp, C.c_int, vp)
    sig("azd_debug_probe_math", C.c_int, C.c_int, vp, vp, C.c_int)
    sig("azd_debug_gemm_bf16", C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, f32p)
    sig("azd_debug_probe_cost", C.c_int, C.c_int, vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, f32p)
    sig("azd_debug_probe_dense_cost", C.c_int, C.c_int, vp, C.c_int, C.c_int, vp, C.c_int, vp, vp, vp, vp)
    sig("azd_dense_ah_cost", C.c_int, vp, C.c_int, C.POINTER(DenseAhCost))
    sig("azd_engine_dense_ah_argmin_data", C.c_int, vp, C.POINTER(DenseAhArgmin))
    sig("azd_engine_dense_ah_agent_cost", C.c_int, vp, C.c_int, C.POINTER(DenseAhCost))
    sig("azd_debug_probe_ah_cost", C.c_int, C.c_int, vp, C.c_int, C.c_int, C.c_int, vp, f32p)
    sig("azd_dense_ah_cost_wide", C.c_int, vp, C.c_int, C.POINTER(DenseAhCost))
    sig("azd_engine_dense_ah_wide_argmin_data", C.c_int, vp, C.POINTER(DenseAhWideArgmin))
    sig("azd_debug_probe_ah_cost_wide", C.c_int, C.c_int, vp, C.c_int, C.c_int, C.c_int, vp, f32p)
    sig("azd_dense_inv_cost", C.c_int, vp, C.c_int, C.POINTER(DenseInvRecipe), C.POINTER(DenseInvCost))
    sig("azd_debug_probe_inv_cost", C.c_int, C.c_int, vp, C.c_int, C.c_int, C.c_int, C.POINTER(DenseInvRecipe), vp, f32p)
    sig("azd_dense_inv_cost_wide", C.c_int, vp, C.c_int, C.POINTER(DenseInvRecipe), C.POINTER(DenseInvCost))
    sig("azd_debug_probe_inv_cost_wide", C.c_int, C.c_int, vp, C.c_int, C.c_int, C.c_int, C.POINTER(DenseInvRecipe), vp, f32p)
    sig("azd_engine_dense_inv_wide_argmin_data", C.c_int, vp, C.POINTER(DenseInvWideArgmin))
    sig("azd_dense_invx_cost", C.c_int, vp, C.c_int, C.POINTER(DenseInvxRecipe), C.POINTER(DenseInvxCost))
    sig("azd_debug_probe_invx_cost", C.c_int, C.c_int, vp, C.c_int, C.c_int, C.c_int, C.POINTER(DenseInvxRecipe), vp, f32p)
    sig("azd_dense_invx_cost_wide", C.c_int, vp, C.c_int, C.POINTER(DenseInvxRecipe), C.POINTER(DenseInvxCost))
    sig("azd_debug_probe_invx_cost_wide", C.c_int, C.c_int, vp, C.c_int, C.c_int, C.c_int, C.POINTER(DenseInvxRecipe), vp, f32p)
    sig("azd_engine_dense_invx_wide_argmin_data", C.c_int, vp, C.POINTER(DenseInvxWideArgmin))
    sig("azd_engine_set_dense_invx_recipe", C.c_int, vp, C.POINTER(DenseInvxRecipe))
    sig("azd_engine_dense_invx_argmin_data", C.c_int, vp, C.POINTER(DenseInvxArgmin))
    sig("azd_engine_dense_invx_agent_cost", C.c_int, vp, C.c_int, C.POINTER(DenseInvxCost))
    sig("azd_dense_invs_cost", C.c_int, vp, C.c_int, C.POINTER(DenseInvsRecipe), C.POINTER(DenseInvsCost))
    sig("azd_dense_invs_spectrum", C.c_int, vp, C.c_int, C.c_int, vp)
    sig("azd_debug_probe_invs_cost", C.c_int, C.c_int, vp, C.c_int, C.c_int, C.c_int, C.POINTER(DenseInvsRecipe), vp, f32p)
    sig("azd_dense_invs_cost_wide", C.c_int, vp, C.c_int, C.POINTER(DenseInvsRecipe), C.POINTER(DenseInvsCost))
    sig("azd_dense_invs_spectrum_wide", C.c_int, vp, C.c_int, C.c_int, vp)
    sig("azd_debug_probe_invs_cost_wide", C.c_int, C.c_int, vp, C.c_int, C.c_int, C.c_int, C.POINTER(DenseInvsRecipe), vp, f32p)
    sig("azd_engine_dense_invs_wide_argmin_data", C.c_int, vp, C.POINTER(DenseInvsWideArgmin))
    sig("azd_engine_set_dense_invs_recipe", C.c_int, vp, C.POINTER(DenseInvsRecipe))
    sig("azd_engine_dense_invs_argmin_data", C.c_int, vp, C.POINTER(DenseInvsArgmin))
    sig("azd_engine_dense_invs_agent_cost", C.c_int, vp, C.c_int, C.POINTER(DenseInvsCost))
    sig("azd_engine_set_dense_inv_recipe", C.c_int, vp, C.POINTER(DenseInvRecipe))
    sig("azd_engine_dense_inv_argmin_data", C.c_int, vp, C.POINTER(DenseInvArgmin))
    sig("azd_engine_dense_inv_agent_cost", C.c_int, vp, C.c_int, C.POINTER(DenseInvCost))
    sig("azd_debug_probe_math_f64", C.c_int, C.c_int, vp, vp, C.c_int)
    _LIB = L
    return L


def check(status, where):
    if status != 0:
        raise AzdError(status, where)


def ptr(a):
    return a.ctypes.data_as(C.c_void_p)
