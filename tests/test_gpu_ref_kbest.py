"""Pins SURVEY row B (KBestList) against the REFERENCE's own device code: tests/golden/
ref_kbest.npz holds what include/ggnn/cuda_utils/k_best_list.cuh of the reference, compiled
unchanged for gfx950 (oracle/ref_kbest_harness.hip), kept of seeded streams on an MI355X
(tests/golden/make_ref_kbest_golden.py).  The oracle's lockstep emulation must reproduce it bit for
bit on random (distance, id) streams with ties, for the block sizes the reference instantiates;
bf_query and top inherit the pin through their own oracle parity tests."""
import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_spec = importlib.util.spec_from_file_location("make_ref_kbest_golden",
                                               os.path.join(GOLDEN, "make_ref_kbest_golden.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)


@pytest.fixture(scope="module")
def ref():
    return np.load(os.path.join(GOLDEN, "ref_kbest.npz"))


@pytest.mark.parametrize("block", [32, 64, 128, 256])
@pytest.mark.parametrize("best", [1, 2, 10, 24, 33, 100, 300])
@pytest.mark.parametrize("check_worst", [True, False])
def test_oracle_kbest_equals_reference_device_code(orc, ref, block, best, check_worst):
    for n, dists, ids in gen.streams(block, best):
        k = gen.key(block, best, check_worst, n)
        rd, ri = ref[k + "_d"], ref[k + "_i"]
        od, oi = orc.kbest_script(best, block, dists, ids, check_worst)
        assert np.array_equal(rd, od), (block, best, n)
        assert np.array_equal(ri, oi), (block, best, n)


def test_engine_bf_query_equals_reference_kbest_order(orc, ref):
    """end to end: the engine's bf_query list == the reference KBestList fed with the exact
    distances in base order (ties keep the lower index first)."""
    from ggnn_amd import ops
    base, q, _ = gen.engine_case()
    ids, d = ops.bf_query(torch.from_numpy(base).cuda(), torch.from_numpy(q).cuda(), gen.ENGINE_K)
    for n in range(q.shape[0]):
        assert np.array_equal(d.cpu().numpy()[n], ref["engine_d"][n])
        assert np.array_equal(ids.cpu().numpy()[n], ref["engine_i"][n])
