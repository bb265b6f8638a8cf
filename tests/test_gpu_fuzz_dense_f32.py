"""A dense-only slice of the differential fuzz of the step forms (tools/fuzz_forms.py, dense_f32=True): random tiers, sizes, key
widths, populations, models, call counts and pool-step knobs; every case runs the same seeded search with an fp32 model in the pool
step (ext_pool_f32=True: the evaluator's gathered fp32 GEMMs) and in the launch-per-phase form, and compares trees, counters, argmin,
improvement counts, state vectors and prediction bits, across an epoch boundary.  A case whose pool step did not run fails."""
import os
import sys

import pytest

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))


def test_twelve_random_dense_cases_with_fp32_models_agree():
    import azdopt_amd
    assert azdopt_amd.device_count() > 0, "no MI355X visible"
    import fuzz_forms
    fuzz_forms.run(12, 16, dense_f32=True)
