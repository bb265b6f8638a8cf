"""bench.py --dump-outputs without a GPU: at the largest shapes the bench runs (config E612: 8192 agents, STATE 3676, ACTION 2450,
trees at their arenas' limits) the files stay float32 / float64 and under 64 MB, and the sample they take is fixed."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402
from azdopt_amd.optimizer import TreeView  # noqa: E402


class _FakeOpt:
    def __init__(self, batch, S, A, nodes, preds):
        self.batch, self.S, self.A, self.nodes, self.preds = batch, S, A, nodes, preds

    def state_vecs(self):
        return np.arange(self.batch * self.S, dtype=np.float32).reshape(self.batch, self.S)

    def predictions(self):
        return np.ones((self.batch, self.A), np.float32)

    def get_tree(self, agent):
        n, p = self.nodes, self.preds
        return TreeView(c=np.full(n, agent, np.float32), c_star=np.zeros(n, np.float32), n_t=np.arange(n, dtype=np.uint32),
                        exhausted=np.zeros(n, np.uint32), e_src=np.zeros(2 * n, np.uint32), p_g=np.full(p, 0.5, np.float32))


class _FakeModel:
    def get_params(self):
        return np.linspace(-1, 1, 3 << 20, dtype=np.float32)


def test_dump_outputs_stays_float_and_under_64_mb_at_the_largest_shapes(tmp_path):
    opt = _FakeOpt(8192, 3676, 2450, nodes=65536, preds=1 << 19)
    written = bench.dump_outputs(str(tmp_path / "a"), opt, _FakeModel(), (0.25, 5.5), [0.1, 0.2])
    assert written <= 64 << 20
    files = sorted(os.listdir(tmp_path / "a"))
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in files) <= 64 << 20
    arrays = {f: np.load(tmp_path / "a" / f) for f in files}
    assert all(a.dtype in (np.float32, np.float64) for a in arrays.values())
    rows = arrays["agent_rows.npy"].astype(np.int64)
    assert 0 < rows.size < 8192 and np.all(np.diff(rows) > 0)
    assert np.array_equal(arrays["state_vecs.npy"], opt.state_vecs()[rows])
    assert arrays["tree_nodes.npy"].shape == (bench.DUMP_TREES * 65536, 4)
    assert arrays["argmin_eval_cost.npy"].tolist() == [0.25, 5.5] and arrays["epoch_losses.npy"].dtype == np.float64
    # the sample is fixed: a second dump of the same outputs writes the same files
    bench.dump_outputs(str(tmp_path / "b"), opt, _FakeModel(), (0.25, 5.5), [0.1, 0.2])
    for f in files:
        assert np.array_equal(arrays[f], np.load(tmp_path / "b" / f)), f


def test_dump_outputs_keeps_every_row_of_the_default_workload(tmp_path):
    opt = _FakeOpt(4096, 304, 152, nodes=1601, preds=40000)
    bench.dump_outputs(str(tmp_path), opt, _FakeModel(), (0.3, 5.9), [])
    assert np.array_equal(np.load(tmp_path / "state_vecs.npy"), opt.state_vecs())
    assert np.load(tmp_path / "epoch_losses.npy").shape == (0,)
    assert np.load(tmp_path / "tree_prediction_g.npy").size == bench.DUMP_TREES * 40000
