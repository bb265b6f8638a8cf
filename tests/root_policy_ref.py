"""Reference of the root policy's options (azd_root_policy): the rule an improved tree keeps nodes by and the weighted colours of
a fresh Ramsey root.  A test helper, not a conftest.

The engines are the existing references -- oracle.py_oracle.PyEngine (c21), oracle.py_ramsey.PyRamseyEngine (Ramsey, recounting)
and tests/ramsey64_ref.Ramsey64RefEngine (Ramsey, any N) -- subclassed: everything but `modify_roots` is inherited.  That method
is the drivers' modify_root closure (04-c21-tree.rs:172-206, 02-r44.rs:196-228) with
  rule "threshold"  an improved tree keeps c <= (c_root + 3 c_root*) / 4          (02-r44.rs:194-196, 04-c21-tree.rs:196-198)
  rule "best"       an improved tree keeps c == c_root*                           (05-r45.rs:201, 03-r3333.rs:191)
and every draw where the unmodified method has it.  tests/test_root_policy_abi.py pins it, with "threshold" and no weights,
against the unmodified oracles before anything is compared with it under the other rule.

Weighted colours (05-r45.rs:84-90: WeightedIndex over the colour probabilities), written from the formula of DESIGN.md ("Seeded
generator"), not from the C++:
  cum_c = cum_{c-1} + w_c in f64, in colour order;  W = cum_{C-1};  T_c = min(2^32, ceil((cum_c / W) * 4294967296.0)), c < C - 1
  colour of a draw r = #{ c < C - 1 : (r >> 32) >= T_c }
Python's float is the same IEEE f64, math.ceil of it an exact integer."""
import math

from oracle import py_oracle as po
from oracle import py_ramsey as pr

import ramsey64_ref as R64

F = po.F
BRANCH_FRESH, BRANCH_STAGNANT, BRANCH_IMPROVED = 0, 1, 2
NO_NODE = 0xFFFFFFFF


def color_thresholds(weights):
    cum, run = [], 0.0
    for w in weights:
        run = run + float(w)
        cum.append(run)
    W = cum[-1]
    return [min(1 << 32, math.ceil((c / W) * 4294967296.0)) for c in cum[:-1]]


def weighted_color(r, thr):
    hi = r >> 32
    return sum(1 for t in thr if hi >= t)


def edge_colors(seed, domain, agent, E, C, color_weights=None):
    """colour of every edge of a fresh root: draw 1024 + e, uniform (below(r, C)) or by the thresholds of `color_weights`"""
    if color_weights is None:
        return [po.below(po.key4(seed, domain, agent, 1024 + e), C) for e in range(E)]
    assert len(color_weights) == C
    thr = color_thresholds(color_weights)
    return [weighted_color(po.key4(seed, domain, agent, 1024 + e), thr) for e in range(E)]


def gen_ramsey_roots(seed, epoch, first_agent, count, n, C, kmin, kmax, color_weights=None):
    """azd_ramsey_generate_roots_weighted restated: list of (colors, permitted edge set)"""
    E = n * (n - 1) // 2
    domain = po.D_ROOT ^ ((epoch << 32) & po.M64)
    out = []
    for i in range(count):
        agent = first_agent + i
        k = kmin + po.below(po.key4(seed, domain, agent, 0), kmax - kmin + 1)
        out.append((edge_colors(seed, domain, agent, E, C, color_weights), po.shuffle_prefix(seed, domain, agent, E, k)))
    return out


class _RootPolicy:
    """modify_roots with a rule and colour weights over the hooks of a space; leaves what it did in self.report:
    per tree (branch, chosen node, size of the kept set)"""

    def modify_roots(self, seed, epoch, first_agent, kmin, kmax, rule="threshold", color_weights=None):
        assert rule in ("threshold", "best")
        domain = po.D_RESET ^ ((epoch << 32) & po.M64)
        out, self.report = [], []
        for i, t in enumerate(self.trees):
            agent = first_agent + i
            r0, r1 = po.key4(seed, domain, agent, 0), po.key4(seed, domain, agent, 1)
            order = sorted(t.pos.items(), key=lambda kv: self.actions_taken(kv[0]))  # BTreeMap order: lexicographic
            c_root, c_root_star = t.node[0]["c"], t.node[0]["cs"]
            kcur = self._permitted_count(i)
            if c_root == c_root_star:
                if kcur == kmax:
                    out.append(self._fresh(seed, domain, agent, kmin + po.below(r1, kmax - kmin + 1), color_weights))
                    self.report.append((BRANCH_FRESH, NO_NODE, 0))
                    continue
                keep = [(k, v) for k, v in order if t.node[v]["c"] == c_root]
                k_new = kcur + po.below(r1, kmax - kcur + 1)
                branch = BRANCH_STAGNANT
            else:
                if rule == "best":
                    keep = [(k, v) for k, v in order if t.node[v]["c"] == c_root_star]
                else:
                    thr = (c_root + F(3.0) * c_root_star) / F(4.0)
                    keep = [(k, v) for k, v in order if t.node[v]["c"] <= thr]
                k_new = kmin + po.below(r1, kmax - kmin + 1)
                branch = BRANCH_IMPROVED
            key, node = keep[po.below(r0, len(keep))]  # an empty `keep` is the reference's unwrap() on None
            out.append(self._replay(i, self.actions_taken(key), po.shuffle_prefix(seed, domain, agent, self._universe(), k_new)))
            self.report.append((branch, node, len(keep)))
        return out


class C21PolicyEngine(_RootPolicy, po.PyEngine):
    def _permitted_count(self, i):
        return len(self.roots[i][1])

    def _universe(self):
        return self.A

    def _fresh(self, seed, domain, agent, k, color_weights):
        assert color_weights is None  # (colour weights are a Ramsey engine's)
        return po.fresh_root(seed, domain, agent, self.n, k)

    def _replay(self, i, actions, new_permitted):
        parents, permitted = list(self.roots[i][0]), set(self.roots[i][1])
        for a in actions:
            po.act(parents, permitted, a)
        return parents, new_permitted


class _RamseyHooks:
    def _permitted_count(self, i):
        return len(self.roots[i].permitted)

    def _universe(self):
        return self.E

    def _fresh(self, seed, domain, agent, k, color_weights):
        return edge_colors(seed, domain, agent, self.E, self.C, color_weights), po.shuffle_prefix(seed, domain, agent, self.E, k)

    def _replay(self, i, actions, new_permitted):
        st = self.roots[i].clone()
        for a in actions:
            st.act(a)
        return list(st.colors), new_permitted


class RamseyPolicyEngine(_RootPolicy, _RamseyHooks, pr.PyRamseyEngine):
    """the recounting reference (N <= 9)"""


class Ramsey64PolicyEngine(_RootPolicy, _RamseyHooks, R64.Ramsey64RefEngine):
    """the reference with maintained counts (any N)"""
