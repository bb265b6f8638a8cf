"""Host-side description of the state/action spaces (the reference's trait surface).

`NablaStateActionSpace` (az-discrete-opt/src/nabla/space/mod.rs:5-39) methods are arbitrary Rust
in the reference; a device engine needs built-in device implementations, selected by id.  The
classes here carry the constants and the host-side closures (`init_states`), nothing more."""
import ctypes as C
import math

import numpy as np

from . import _lib


class ActionsNeverRepeat:
    """Marker: az-discrete-opt/src/space/axioms.rs:7"""


class ActionOrderIndependent:
    """Marker: az-discrete-opt/src/space/axioms.rs:10"""


class ActionSet:
    """Path encoding keyed by the SET of actions taken (az-discrete-opt/src/path/set.rs:6-37).
    Licensed only for spaces that are ActionsNeverRepeat + ActionOrderIndependent
    (space/axioms.rs:16-19).  On the device it is a KW x u64 bit mask per node."""
    PATH_KIND = _lib.PATH_SET

    @staticmethod
    def licensed_for(space):
        return isinstance(space, ActionsNeverRepeat) and isinstance(space, ActionOrderIndependent)


class ActionMultiset:
    """Path encoding keyed by the multiset of actions (path/multiset.rs:5-42), licensed for
    ActionOrderIndependent spaces (axioms.rs:14).  On a space that is also ActionsNeverRepeat every
    multiplicity is 1, so identity, order and length coincide with ActionSet's: same device keys."""
    PATH_KIND = _lib.PATH_SET

    @staticmethod
    def licensed_for(space):
        return isinstance(space, ActionOrderIndependent) and isinstance(space, ActionsNeverRepeat)


class ActionSequence:
    """Path encoding keyed by the actions in the order taken (path/sequence.rs:3-36), licensed for
    every space.  Distinct orders are distinct nodes: no transpositions, the search graph is a tree."""
    PATH_KIND = _lib.PATH_SEQUENCE

    @staticmethod
    def licensed_for(space):
        return True


class OrderedActionSet(ActionSequence):
    """path/ord_set.rs:3-34: despite the name a Vec that push_unchecked appends to, i.e. the same
    key as ActionSequence; licensed for ActionsNeverRepeat spaces (axioms.rs:12)."""

    @staticmethod
    def licensed_for(space):
        return isinstance(space, ActionsNeverRepeat)


class ROTModifyParentsOnce(ActionsNeverRepeat, ActionOrderIndependent):
    """c21 space: rooted ordered trees on N vertices, each parent may be modified once
    (graph-state/src/rooted_tree/space.rs:14-125; axioms asserted at :124-125).
    cost = Conjecture2Dot1Cost {lambda_1, matching}; evaluate = squish(mu + lambda_1)
    (graph-state/examples/04-c21-tree.rs:58-74,96-105)."""

    SPACE_ID = _lib.SPACE_C21

    def __init__(self, n):
        self.n = int(n)
        L = _lib.lib()
        self.STATE_DIM = L.azd_c21_state_dim(self.n)    # space.rs:46
        self.ACTION_DIM = L.azd_c21_action_dim(self.n)  # space.rs:48
        self.KEY_WORDS = L.azd_c21_key_words(self.n)

    @property
    def ROOT_BYTES(self):
        return self.n

    def default_permitted_range(self):
        """04-c21-tree.rs:85: 5..=(ACTION / 2), clamped for tiny N"""
        hi = max(1, self.ACTION_DIM // 2)
        return min(5, hi), hi

    def generate_roots(self, seed, count, first_agent=0, epoch=0, kmin=None, kmax=None):
        """`init_states` of the driver (04-c21-tree.rs:108-112) with a seeded generator.
        Returns packed roots: parents u8 [count, n], permitted u64 [count, KEY_WORDS]."""
        lo, hi = self.default_permitted_range()
        kmin = lo if kmin is None else kmin
        kmax = hi if kmax is None else kmax
        parents = np.zeros((count, self.n), np.uint8)
        permitted = np.zeros((count, self.KEY_WORDS), np.uint64)
        _lib.check(_lib.lib().azd_c21_generate_roots(seed, epoch, first_agent, count, self.n, kmin, kmax,
                                                     _lib.ptr(parents), _lib.ptr(permitted)), "azd_c21_generate_roots")
        return parents, permitted

    @staticmethod
    def action(index):
        """(parent, child) of action `index` (ordered_edge.rs:40-42 via edge.rs:55-65)"""
        c = 2
        while c * (c + 1) // 2 - 1 <= index:
            c += 1
        return index - (c * (c - 1) // 2 - 1), c


class RamseySpaceNoEdgeRecolor(ActionsNeverRepeat, ActionOrderIndependent):
    """Ramsey space: C-colourings of the edges of K_N, an action recolours one still-permitted edge
    (graph-state/src/ramsey_counts/space.rs:10-176; axioms asserted at :179-186).
    cost = TotalCounts (monochromatic `sizes[c]`-cliques per colour); evaluate = sum_c count_c * w_c;
    g = c_s h + r (1 - h), h_sa = 1 - c*/c (:159-177).  Drivers: 01-r333.rs (N 16, [3,3,3]),
    02-r44.rs (N 17, [4,4])."""

    SPACE_ID = _lib.SPACE_RAMSEY

    def __init__(self, n, sizes, weights=None, max_slots=None, u64=None, big_cliques=None):
        """`max_slots`: the most permitted edges a root may bring.  0 keeps the engine's narrow limits (E <= 256, E*C <= 384,
        at most 128 / (C - 1) permitted edges); 1..E makes it a WIDE engine (N <= 32, E*C <= 1024; a node holds up to
        max_slots * (C - 1) legal actions).  None: 0 where the narrow limits hold, else E -- every edge may be permitted,
        as 05-r45.rs:83 allows.
        `u64`: the 64-bit tier (N <= 64, E*C <= 2304, max_slots * (C - 1) <= 512; 03-r3333.rs: N = 34, four colours).  None: only
        where neither 32-bit tier takes the shape; True forces it (any shape it takes), False forbids it.  With it, max_slots = None
        is as many edges as a node of 512 actions holds, at most E.
        `big_cliques`: clique sizes up to 8 on the 64-bit tier (ENGINE_RAMSEY_BIG_CLIQUES: kernels of their own).  None: exactly when
        a size exceeds 5, and the 64-bit tier is then forced; True forces it (any shape the tier takes, the same trees); a size
        above 5 with u64=False or big_cliques=False raises ValueError.  With it every colour must pass the reference's i32 bound
        (RamseyCounts::new, ramsey_counts/mod.rs:47-62, sums before it divides): C(s,2) * C(n,s) <= 2^31 - 1."""
        self.n = int(n)
        self.sizes = [int(x) for x in sizes]
        self.weights = [1.0] * len(self.sizes) if weights is None else [float(x) for x in weights]
        self.C = len(self.sizes)
        self.E = self.n * (self.n - 1) // 2
        L = _lib.lib()
        self.STATE_DIM = L.azd_ramsey_state_dim(self.n, self.C)    # space.rs:40
        self.ACTION_DIM = L.azd_ramsey_action_dim(self.n, self.C)  # space.rs:42
        self.KEY_WORDS = L.azd_ramsey_key_words(self.n, self.C)
        if max(self.sizes) > 5 and (u64 is False or big_cliques is False):
            raise ValueError("clique sizes above 5 need the 64-bit tier with big_cliques (u64=%r, big_cliques=%r)" % (u64, big_cliques))
        if big_cliques is None:
            big_cliques = max(self.sizes) > 5
        if big_cliques and u64 is False:
            raise ValueError("big_cliques needs the 64-bit tier (u64=False)")
        self.BIG_CLIQUES = bool(big_cliques)
        if self.BIG_CLIQUES:
            u64 = True
            for c, s_ in enumerate(self.sizes):
                if 2 <= s_ <= _lib.RAMSEY_BIG_CLIQUE_MAX and math.comb(s_, 2) * math.comb(self.n, s_) > 2 ** 31 - 1:
                    raise ValueError("colour %d (clique size %d at n = %d) is beyond the reference's i32 bound: C(s,2) * C(n,s) <= 2^31 - 1"
                                     % (c, s_, self.n))
        if u64 is None:
            u64 = self.n > _lib.RAMSEY_WIDE_MAX_N or self.ACTION_DIM > 1024
        self.U64 = bool(u64)
        if max_slots is None:
            narrow = self.n <= _lib.RAMSEY_MAX_N and self.E <= 256 and self.KEY_WORDS <= 6
            if self.U64:
                max_slots = min(self.E, _lib.RAMSEY_U64_NODE_ACTIONS // (self.C - 1))
            else:
                max_slots = 0 if narrow else self.E
        self.MAX_SLOTS = int(max_slots)

    @property
    def ROOT_BYTES(self):
        return self.E

    @property
    def wide(self):
        return self.MAX_SLOTS > 0

    @property
    def tier(self):
        """"narrow" (E <= 256, E*C <= 384), "wide" (N <= 32, E*C <= 1024) or "u64" (N <= 64, E*C <= 2304; with BIG_CLIQUES sizes up to 8)"""
        return "u64" if self.U64 else "wide" if self.wide else "narrow"

    def default_permitted_range(self):
        """02-r44.rs:83: 12..=(E / 2), clamped to what one node can hold (max_slots edges on a wide engine)"""
        cap = self.MAX_SLOTS if self.wide else 128 // (self.C - 1)
        hi = max(1, min(self.E // 2, cap))
        return min(12, hi), hi

    def generate_roots(self, seed, count, first_agent=0, epoch=0, kmin=None, kmax=None, color_weights=None):
        """`init_state` of the drivers with a seeded generator.  Returns packed roots:
        colors u8 [count, E], permitted edges u64 [count, KEY_WORDS].
        color_weights: the colour probabilities of 05-r45.rs:84-90 (WeightedIndex), one per colour; None: uniform colours."""
        lo, hi = self.default_permitted_range()
        kmin = lo if kmin is None else kmin
        kmax = hi if kmax is None else kmax
        colors = np.zeros((count, self.E), np.uint8)
        permitted = np.zeros((count, self.KEY_WORDS), np.uint64)
        w = None
        if color_weights is not None:
            w = np.ascontiguousarray(color_weights, np.float64)
            if w.shape != (self.C,):
                raise ValueError("color_weights: one weight per colour")
        _lib.check(_lib.lib().azd_ramsey_generate_roots_weighted(seed, epoch, first_agent, count, self.n, self.C, kmin, kmax,
                                                                 None if w is None else _lib.ptr(w), _lib.ptr(colors),
                                                                 _lib.ptr(permitted)), "azd_ramsey_generate_roots_weighted")
        return colors, permitted

    def action(self, index):
        """(edge position, new colour) of action `index` (space.rs:48-54)"""
        return index % self.E, index // self.E


class InvariantCost:
    """A recipe of the dense-graph space's weighted-invariant cost (AZD_ENGINE_DENSE_INV; azd_dense_inv_recipe): a linear
    combination of ten invariants of a connected graph, chosen at run time --
        edges, max_degree, min_degree, diameter, radius, proximity, remoteness, avg_distance,
        adj_eig (adjacency eigenvalue at descending index adj_index), dist_eig (distance-matrix eigenvalue at descending index
        dist_index, or "ah": floor(2D/3) - 1, n - 1 when floor(2D/3) = 0)
    cost = (f32)(bias + sum of weight * invariant, in that order, over the non-zero weights); eval = eval_scale * (cost + eval_offset).
    A spectral invariant with weight 0 is not computed.  `weights`: dict name -> weight (names not given weigh 0)."""

    NAMES = _lib.DENSE_INV_NAMES

    def __init__(self, weights, bias=0.0, adj_index=0, dist_index="ah", eval_offset=0.0, eval_scale=1.0):
        unknown = sorted(set(weights) - set(self.NAMES))
        if unknown:
            raise ValueError("unknown invariant(s) %s: the names are %s" % (", ".join(unknown), ", ".join(self.NAMES)))
        self.weights = {k: float(v) for k, v in weights.items()}
        self.bias, self.adj_index = float(bias), int(adj_index)
        self.dist_index = _lib.DENSE_INV_INDEX_AH if dist_index in ("ah", None) else int(dist_index)
        self.eval_offset, self.eval_scale = np.float32(eval_offset), np.float32(eval_scale)

    @classmethod
    def aouchiche_hansen(cls, n):
        """the recipe whose cost and eval are the Aouchiche-Hansen cost's (cost="ah") bit for bit"""
        return cls({"proximity": 1.0, "dist_eig": 1.0}, dist_index="ah", eval_offset=2.0, eval_scale=np.float32(1.0) / np.float32(2 * n + 2))

    @classmethod
    def from_dict(cls, d):
        """from a JSON object: {"weights": {...}, "bias": .., "adj_index": .., "dist_index": .. | "ah", "eval_offset": .., "eval_scale": ..}"""
        return cls(d["weights"], **{k: d[k] for k in ("bias", "adj_index", "dist_index", "eval_offset", "eval_scale") if k in d})

    def recipe(self):
        r = _lib.DenseInvRecipe()
        for i, name in enumerate(self.NAMES):
            r.weight[i] = self.weights.get(name, 0.0)
        r.bias, r.adj_index, r.dist_index = self.bias, self.adj_index, self.dist_index
        r.eval_offset, r.eval_scale = float(self.eval_offset), float(self.eval_scale)
        return r

    @classmethod
    def record(cls, rec):
        """an azd_dense_inv_cost_t (or the cost part of an argmin record) as a dict: the invariants by name, dist_k, computed, cost"""
        out = {name: rec.inv[i] for i, name in enumerate(cls.NAMES)}
        out.update(dist_k=rec.dist_k, computed=rec.computed, cost=np.float32(rec.cost))
        return out


class InvariantCostX:
    """A recipe of the dense-graph space's extended invariant cost (AZD_ENGINE_DENSE_INVX; azd_dense_invx_recipe): sixteen
    invariants of a connected graph -- InvariantCost's ten, then
        lap_eig (eigenvalue of D - A at descending index lap_index; n - 2 is the algebraic connectivity), slap_eig (of D + A at
        slap_index), randic, zagreb1, zagreb2, triangles
    -- combined with weights and up to four pair terms `terms=[(coef, "a", "*" | "/", "b"), ...]`:
    cost = (f32)(bias + sum of weight * invariant over the non-zero weights, in order, + sum of coef * (a * b or a / b), in order);
    eval = eval_scale * (cost + eval_offset).  A divisor is one of the invariants that are positive on every connected graph
    (DIVISORS).  An eigenvalue, randic, a Zagreb index or the triangle count is computed only when a non-zero weight or coefficient
    asks for it.  With no such weight and no term it is InvariantCost's cost, bit for bit."""

    NAMES = _lib.DENSE_INVX_NAMES
    DIVISORS = _lib.DENSE_INVX_NAMES[:8] + ("randic", "zagreb1", "zagreb2")
    OPS = {"*": _lib.DENSE_INVX_MUL, "/": _lib.DENSE_INVX_DIV}

    def __init__(self, weights, terms=(), bias=0.0, adj_index=0, dist_index="ah", lap_index=0, slap_index=0, eval_offset=0.0, eval_scale=1.0):
        terms = [(float(c), str(a), str(op), str(b)) for c, a, op, b in terms]
        unknown = sorted((set(weights) | {x for _, a, _, b in terms for x in (a, b)}) - set(self.NAMES))
        if unknown:
            raise ValueError("unknown invariant(s) %s: the names are %s" % (", ".join(unknown), ", ".join(self.NAMES)))
        if len(terms) > _lib.DENSE_INVX_MAX_TERMS:
            raise ValueError("terms: at most %d pair terms" % _lib.DENSE_INVX_MAX_TERMS)
        for _, _, op, b in terms:
            if op not in self.OPS:
                raise ValueError('terms: the operation is "*" or "/", not %r' % (op,))
            if op == "/" and b not in self.DIVISORS:
                raise ValueError("terms: %s cannot divide (it can be zero); the divisors are %s" % (b, ", ".join(self.DIVISORS)))
        self.weights = {k: float(v) for k, v in weights.items()}
        self.terms = terms
        self.bias, self.adj_index, self.lap_index, self.slap_index = float(bias), int(adj_index), int(lap_index), int(slap_index)
        self.dist_index = _lib.DENSE_INV_INDEX_AH if dist_index in ("ah", None) else int(dist_index)
        self.eval_offset, self.eval_scale = np.float32(eval_offset), np.float32(eval_scale)

    @classmethod
    def from_invariant_cost(cls, cost):
        """the recipe that gives an InvariantCost's cost, eval and trees bit for bit"""
        return cls(cost.weights, bias=cost.bias, adj_index=cost.adj_index, dist_index=cost.dist_index, eval_offset=cost.eval_offset,
                   eval_scale=cost.eval_scale)

    @classmethod
    def from_dict(cls, d):
        """from a JSON object: {"weights": {...}, "terms": [[coef, "a", "*" | "/", "b"], ...], "bias": .., "adj_index": ..,
        "dist_index": .. | "ah", "lap_index": .., "slap_index": .., "eval_offset": .., "eval_scale": ..}"""
        keys = ("terms", "bias", "adj_index", "dist_index", "lap_index", "slap_index", "eval_offset", "eval_scale")
        return cls(d.get("weights", {}), **{k: d[k] for k in keys if k in d})

    def recipe(self):
        r = _lib.DenseInvxRecipe()
        for i, name in enumerate(self.NAMES):
            r.weight[i] = self.weights.get(name, 0.0)
        r.bias, r.adj_index, r.dist_index, r.lap_index, r.slap_index = self.bias, self.adj_index, self.dist_index, self.lap_index, self.slap_index
        r.eval_offset, r.eval_scale = float(self.eval_offset), float(self.eval_scale)
        for t, (coef, a, op, b) in enumerate(self.terms):
            r.term[t].coef, r.term[t].a, r.term[t].b, r.term[t].op = coef, self.NAMES.index(a), self.NAMES.index(b), self.OPS[op]
        r.n_terms = len(self.terms)
        return r

    @classmethod
    def record(cls, rec):
        """an azd_dense_invx_cost_t (or the cost part of an argmin record) as a dict: the invariants by name, dist_k, computed, cost"""
        out = {name: rec.inv[i] for i, name in enumerate(cls.NAMES)}
        out.update(dist_k=rec.dist_k, computed=rec.computed, cost=np.float32(rec.cost))
        return out


class InvariantCostS(InvariantCostX):
    """A recipe of the dense-graph space's spectrum invariant cost (AZD_ENGINE_DENSE_INVS; azd_dense_invs_recipe): twenty-one
    invariants of a connected graph -- InvariantCostX's sixteen, then functions of a matrix's WHOLE spectrum:
        adj_energy (the graph energy, sum of |eigenvalue| of A), dist_energy (of the distance matrix), lap_energy and slap_energy
        (sum of |eigenvalue - mean degree| of D - A and D + A), adj_spread (largest minus smallest eigenvalue of A)
    -- combined by InvariantCostX's rule.  All five are positive on every connected graph and may divide.  A matrix is reduced once;
    its one eigenvalue by index and its energy are each computed only when a non-zero weight or coefficient asks for it.  With none
    of the five asked for it is InvariantCostX's cost, bit for bit."""

    NAMES = _lib.DENSE_INVS_NAMES
    DIVISORS = InvariantCostX.DIVISORS + _lib.DENSE_INVS_NAMES[16:]

    @classmethod
    def from_invariant_cost_x(cls, cost):
        """the recipe that gives an InvariantCostX's cost, eval and trees bit for bit"""
        return cls(cost.weights, terms=cost.terms, bias=cost.bias, adj_index=cost.adj_index, dist_index=cost.dist_index, lap_index=cost.lap_index,
                   slap_index=cost.slap_index, eval_offset=cost.eval_offset, eval_scale=cost.eval_scale)

    def recipe(self):
        r = _lib.DenseInvsRecipe()
        for i, name in enumerate(self.NAMES):
            r.weight[i] = self.weights.get(name, 0.0)
        r.bias, r.adj_index, r.dist_index, r.lap_index, r.slap_index = self.bias, self.adj_index, self.dist_index, self.lap_index, self.slap_index
        r.eval_offset, r.eval_scale = float(self.eval_offset), float(self.eval_scale)
        for t, (coef, a, op, b) in enumerate(self.terms):
            r.term[t].coef, r.term[t].a, r.term[t].b, r.term[t].op = coef, self.NAMES.index(a), self.NAMES.index(b), self.OPS[op]
        r.n_terms = len(self.terms)
        return r


class DenseGraphSpace(ActionsNeverRepeat, ActionOrderIndependent):
    """Connected graphs on N <= 64 vertices; an action adds an absent edge or deletes a present non-cut edge, every edge
    slot at most once (BASELINE configs[4], N = 50).  BUILD-DEFINED: the reference has the pieces
    (connected_bitset_graph/mod.rs: is_cut_edge, action_kinds, conjecture_2_1_cost; bitset_graph/space/action.rs:
    AddOrDeleteEdge indexing; 05-ah.rs:39-40: STATE = E + ACTION + 1) but no live NablaStateActionSpace over general
    graphs; the definition is in oracle/dense_graph.inc.  cost = Conjecture2Dot1Cost {lambda_1, matching number};
    evaluate = squish(mu + lambda_1) with the bounds of 04-c21-tree.rs:58-74.  `max_slots`: the most modifiable slots a root
    may bring (= legal actions a node can hold; the engine sizes its keys from it: 128 / 256 / 640 / 1024); the drivers'
    image is E // 2 (04-c21-tree.rs:85 permits up to half of ACTION_DIM), 128 keeps the keys at two words.
    `cost`: "c21" (the default, above) or "ah" -- the Aouchiche-Hansen cost, the objective of the reference's 05-ah.rs
    (ConnectedBitsetGraph::ah_cost, mod.rs:156-198): proximity + the distance matrix's eigenvalue of index floor(2D/3) - 1;
    BUILD-DEFINED evaluate = (cost + 2) / (2N + 2).  N <= 32 there (AZD_ENGINE_DENSE_AH); states, actions, keys and roots are the
    same space's.  `ah_wide=True` (with cost="ah" only): the cost's 64-row form, N <= 64 (AZD_ENGINE_DENSE_AH_WIDE beside the
    first flag; never chosen from N), roots of at most min(E, 640) slots; at N <= 32 it gives what the narrow form gives.
    `cost=InvariantCost(...)`: the weighted-invariant cost (AZD_ENGINE_DENSE_INV, N <= 32, the AH tier's limits): a linear
    combination of ten graph invariants whose weights are given here, at run time; NablaOptimizer.par_new hands the recipe to
    the engine.  InvariantCost.aouchiche_hansen(n) is the recipe that gives cost="ah"'s trees.  `inv_wide=True` (with an
    InvariantCost only): that cost's 64-row form, N <= 64 (AZD_ENGINE_DENSE_INV_WIDE beside the first flag; never chosen from N),
    roots of at most min(E, 640) slots; at N <= 32 it gives what the narrow form gives.
    `cost=InvariantCostX(...)`: the extended invariant cost (AZD_ENGINE_DENSE_INVX, N <= 32, a tier of its own with the
    InvariantCost tier's limits): sixteen invariants -- Laplacian and signless-Laplacian eigenvalues, Randic and Zagreb indices and
    the triangle count beside the ten -- and products or quotients of two of them.  InvariantCostX.from_invariant_cost(c) gives
    cost=c's trees.  `invx_wide=True` (with an InvariantCostX only): that cost's 64-row form, N <= 64 (AZD_ENGINE_DENSE_INVX_WIDE
    beside the first flag; never chosen from N), roots of at most min(E, 640) slots; at N <= 32 it gives what the narrow form gives.
    `cost=InvariantCostS(...)`: the spectrum invariant cost (AZD_ENGINE_DENSE_INVS, N <= 32, a tier of its own with the
    InvariantCostX tier's limits): the graph energy, the distance, Laplacian and signless-Laplacian energies and the adjacency spread
    beside the sixteen.  InvariantCostS.from_invariant_cost_x(c) gives cost=c's trees.  `invs_wide=True` (with an InvariantCostS
    only): that cost's 64-row form, N <= 64 (AZD_ENGINE_DENSE_INVS_WIDE beside the first flag; never chosen from N), roots of at most
    min(E, 640) slots; at N <= 32 it gives what the narrow form gives.  Neither form has a pool step."""

    SPACE_ID = _lib.SPACE_DENSE

    def __init__(self, n, p=0.2, max_slots=128, cost="c21", ah_wide=False, inv_wide=False, invx_wide=False, invs_wide=False):
        self.INV = cost if isinstance(cost, InvariantCost) else None
        self.INVS = cost if isinstance(cost, InvariantCostS) else None
        self.INVX = cost if isinstance(cost, InvariantCostX) and self.INVS is None else None
        if self.INV is not None:
            cost = "inv"
        elif self.INVS is not None:
            cost = "invs"
        elif self.INVX is not None:
            cost = "invx"
        elif cost not in ("c21", "ah"):
            raise ValueError('cost must be "c21", "ah", an InvariantCost, an InvariantCostX or an InvariantCostS')
        if ah_wide and cost != "ah":
            raise ValueError('ah_wide=True needs cost="ah" (it is the Aouchiche-Hansen cost\'s 64-row form)')
        if inv_wide and cost != "inv":
            raise ValueError("inv_wide=True needs cost=InvariantCost(...) (it is the weighted-invariant cost's 64-row form)")
        if invx_wide and cost != "invx":
            raise ValueError("invx_wide=True needs cost=InvariantCostX(...) (it is the extended invariant cost's 64-row form)")
        if invs_wide and cost != "invs":
            raise ValueError("invs_wide=True needs cost=InvariantCostS(...) (it is the spectrum invariant cost's 64-row form)")
        self.COST = cost
        self.AH_WIDE = bool(ah_wide)
        self.INV_WIDE = bool(inv_wide)
        self.INVX_WIDE = bool(invx_wide)
        self.INVS_WIDE = bool(invs_wide)
        self.n, self.p = int(n), float(p)
        self.E = self.n * (self.n - 1) // 2
        # (an AZD_ENGINE_DENSE_AH engine refuses max_slots > E; a root cannot bring more than E slots anyway)
        # (... and an AZD_ENGINE_DENSE_AH_WIDE, AZD_ENGINE_DENSE_INV_WIDE, AZD_ENGINE_DENSE_INVX_WIDE or AZD_ENGINE_DENSE_INVS_WIDE engine
        # max_slots > min(E, 640): its keys are 2, 4 or 10 words)
        self.MAX_SLOTS = min(int(max_slots), self.E, 640) if ah_wide or inv_wide or invx_wide or invs_wide else min(int(max_slots), self.E) if cost in ("ah", "inv", "invx", "invs") else int(max_slots)
        L = _lib.lib()
        self.STATE_DIM = L.azd_dense_state_dim(self.n)
        self.ACTION_DIM = L.azd_dense_action_dim(self.n)
        self.KEY_WORDS = L.azd_dense_key_words(self.n)

    @property
    def ROOT_BYTES(self):
        return 8 * self.n

    def default_permitted_range(self):
        hi = min(self.MAX_SLOTS, self.E // 2)
        return min(5, hi), hi

    def generate_roots(self, seed, count, first_agent=0, epoch=0, kmin=None, kmax=None):
        """seeded `init_states`: (adj u64 [count, n] viewed as bytes [count, 8 n], modifiable slots u64 [count, KEY_WORDS])"""
        lo, hi = self.default_permitted_range()
        kmin = lo if kmin is None else kmin
        kmax = hi if kmax is None else kmax
        adj = np.zeros((count, self.n), np.uint64)
        slots = np.zeros((count, self.KEY_WORDS), np.uint64)
        _lib.check(_lib.lib().azd_dense_generate_roots(seed, epoch, first_agent, count, self.n, kmin, kmax, self.p,
                                                       _lib.ptr(adj), _lib.ptr(slots)), "azd_dense_generate_roots")
        return adj.view(np.uint8).reshape(count, 8 * self.n), slots

    def action(self, index):
        """("add" | "delete", edge slot) of action `index` (AddOrDeleteEdge::from_action_index, action.rs:20-27)"""
        return ("add", index) if index < self.E else ("delete", index - self.E)

    def ah_cost(self, adj):
        """The Aouchiche-Hansen cost of one connected graph (n neighbourhood bitsets) on the host: azd_dense_ah_cost
        (azd_dense_ah_cost_wide for an ah_wide space), the same procedure as the device's, bit for bit.
        -> dict(proximity, eigenvalue, diameter, k, cost, eval)"""
        a = np.ascontiguousarray(adj, np.uint64).reshape(self.n)
        out = _lib.DenseAhCost()
        if getattr(self, "AH_WIDE", False):
            _lib.check(_lib.lib().azd_dense_ah_cost_wide(_lib.ptr(a), self.n, C.byref(out)), "azd_dense_ah_cost_wide")
        else:
            _lib.check(_lib.lib().azd_dense_ah_cost(_lib.ptr(a), self.n, C.byref(out)), "azd_dense_ah_cost")
        return dict(proximity=out.proximity, eigenvalue=out.eigenvalue, diameter=out.diameter, k=out.k,
                    cost=np.float32(out.cost), eval=np.float32(out.eval))

    def inv_cost(self, adj, cost=None):
        """The weighted-invariant cost of one connected graph (n neighbourhood bitsets) on the host: azd_dense_inv_cost
        (azd_dense_inv_cost_wide for an inv_wide space) under this space's recipe (or `cost`, another InvariantCost), the same
        procedure as the device's, bit for bit.
        -> dict(the ten invariants by name, dist_k, computed, cost, eval)"""
        cost = self.INV if cost is None else cost
        if cost is None:
            raise ValueError("inv_cost: the space has no InvariantCost; pass one")
        a = np.ascontiguousarray(adj, np.uint64).reshape(self.n)
        out, r = _lib.DenseInvCost(), cost.recipe()
        if getattr(self, "INV_WIDE", False):
            _lib.check(_lib.lib().azd_dense_inv_cost_wide(_lib.ptr(a), self.n, C.byref(r), C.byref(out)), "azd_dense_inv_cost_wide")
        else:
            _lib.check(_lib.lib().azd_dense_inv_cost(_lib.ptr(a), self.n, C.byref(r), C.byref(out)), "azd_dense_inv_cost")
        return dict(InvariantCost.record(out), eval=np.float32(out.eval))

    def invx_cost(self, adj, cost=None):
        """The extended invariant cost of one connected graph (n neighbourhood bitsets) on the host: azd_dense_invx_cost
        (azd_dense_invx_cost_wide for an invx_wide space) under this space's recipe (or `cost`, another InvariantCostX), the same
        procedure as the device's, bit for bit.
        -> dict(the sixteen invariants by name, dist_k, computed, cost, eval)"""
        cost = self.INVX if cost is None else cost
        if cost is None:
            raise ValueError("invx_cost: the space has no InvariantCostX; pass one")
        a = np.ascontiguousarray(adj, np.uint64).reshape(self.n)
        out, r = _lib.DenseInvxCost(), cost.recipe()
        if getattr(self, "INVX_WIDE", False):
            _lib.check(_lib.lib().azd_dense_invx_cost_wide(_lib.ptr(a), self.n, C.byref(r), C.byref(out)), "azd_dense_invx_cost_wide")
        else:
            _lib.check(_lib.lib().azd_dense_invx_cost(_lib.ptr(a), self.n, C.byref(r), C.byref(out)), "azd_dense_invx_cost")
        return dict(InvariantCostX.record(out), eval=np.float32(out.eval))

    def invs_cost(self, adj, cost=None):
        """The spectrum invariant cost of one connected graph (n neighbourhood bitsets) on the host: azd_dense_invs_cost
        (azd_dense_invs_cost_wide for an invs_wide space) under this space's recipe (or `cost`, another InvariantCostS), the same
        procedure as the device's, bit for bit.
        -> dict(the twenty-one invariants by name, dist_k, computed, cost, eval)"""
        cost = self.INVS if cost is None else cost
        if cost is None:
            raise ValueError("invs_cost: the space has no InvariantCostS; pass one")
        a = np.ascontiguousarray(adj, np.uint64).reshape(self.n)
        out, r = _lib.DenseInvsCost(), cost.recipe()
        if getattr(self, "INVS_WIDE", False):
            _lib.check(_lib.lib().azd_dense_invs_cost_wide(_lib.ptr(a), self.n, C.byref(r), C.byref(out)), "azd_dense_invs_cost_wide")
        else:
            _lib.check(_lib.lib().azd_dense_invs_cost(_lib.ptr(a), self.n, C.byref(r), C.byref(out)), "azd_dense_invs_cost")
        return dict(InvariantCostS.record(out), eval=np.float32(out.eval))

    def invs_spectrum(self, adj, which="adj"):
        """All eigenvalues, ascending, of the graph's adjacency ("adj"), distance ("dist"), Laplacian ("lap") or signless-Laplacian
        ("slap") matrix by the cost's whole-spectrum procedure on the host (azd_dense_invs_spectrum; azd_dense_invs_spectrum_wide for an
        invs_wide space): what the energies sum."""
        a = np.ascontiguousarray(adj, np.uint64).reshape(self.n)
        out = np.zeros(self.n, np.float64)
        wide = getattr(self, "INVS_WIDE", False)
        fn = _lib.lib().azd_dense_invs_spectrum_wide if wide else _lib.lib().azd_dense_invs_spectrum
        _lib.check(fn(_lib.ptr(a), self.n, ("adj", "dist", "lap", "slap").index(which), _lib.ptr(out)), "azd_dense_invs_spectrum_wide" if wide else "azd_dense_invs_spectrum")
        return out


class Layered:
    """Layered<LAYERS, Space> (az-discrete-opt/src/space/layered.rs:3-20; trait impl nabla/space/mod.rs:41-111):
    the evaluator sees the last `layers` states of the path.  STATE_DIM = layers * inner STATE_DIM; every other
    method is the inner space's on the newest state; the axioms are inherited (layered.rs:12-19)."""

    def __init__(self, space, layers):
        if not 2 <= int(layers) <= 8:
            raise ValueError("layers must be 2..8")
        self.space, self.layers = space, int(layers)
        self.STATE_DIM = space.STATE_DIM * self.layers  # nabla/space/mod.rs:53
        # marker axioms follow the inner space
        self.__class__ = type("Layered", (Layered,) + tuple(b for b in (ActionsNeverRepeat, ActionOrderIndependent)
                                                            if isinstance(space, b)), {})

    def __getattr__(self, name):  # ACTION_DIM, KEY_WORDS, n, SPACE_ID, generate_roots, ...
        return getattr(self.space, name)
