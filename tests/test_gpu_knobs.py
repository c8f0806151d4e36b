"""The knob surface of qn_debug_set: the keys that exist are accepted, the retired ones are unknown keys like any other, and setting
every knob to its documented default changes nothing - a context that never had a knob set runs the same registration bit for bit."""
import numpy as np
import pytest
from qn_amd import synth

pytestmark = pytest.mark.gpu

# key -> documented default (csrc/qn_context.h).  The probes and the debug modes allocate device scratch when switched on: off is their default.
SURVIVING = {
    "cell": 0, "device_look": 1, "far_group": -1, "tgt_early": 1, "c2f_lanes_fpfh": 0, "normals_fg": 0, "fpfh_fg": 0, "far_ranked": 1, "pair_pipeline": 1,
    "persist": 1, "persist_timeout": 25000000, "prof_persist": 0, "persist_probe": 0, "batch_lanes": 8, "fail_lane_create": 0, "batch_share_source": 1,
    "batch_trace": 0, "batch_member": 0, "knn_hist": 1, "nn_lane": -1, "track_from_tick": 3, "single_from_tick": 2, "knn_trips": 3, "knn_mm": 1,
    "dbg_counters": 0, "far": 1, "feat_mfma": 1, "feat_sample": 4, "feat_query_dedupe": 0, "feat_verify": 0, "list_probe": 0, "clk_probe": 0, "tick_rpb": 2,
    "batch_min_share": 4, "verify_track": 0,
}
ALLOCATING_OR_PROBE = ("persist_probe", "dbg_counters", "list_probe", "clk_probe", "verify_track")
RETIRED = (
    "margin_nn", "margin_nn_t0", "margin_knn", "margin_nn_cap", "margin_knn_cap", "big_blocks0", "fb_blocks0", "big_ratio", "knn_single_all", "bbox_blocks",
    "c2f_overlap", "quatro_fused", "list_small", "far_chunk", "batch_look", "unseeded_cap", "stable_cells", "nn_rounds", "knn_rounds", "fused_from_tick",
    "fused_ticks", "fused_final", "ticks_per_chunk", "tick_occ", "tick_tb", "tick_ppt_min", "tick_lds_pad", "knn_lds_pad", "feat_min_blocks",
)


@pytest.fixture(scope="module")
def ctx():
    from qn_amd import engine
    c = engine.Context(1024)
    yield c
    c.close()


def test_key_lists_are_what_they_claim():
    assert len(SURVIVING) == 35 and len(RETIRED) == 29 and len(set(RETIRED)) == 29 and not set(RETIRED) & set(SURVIVING)
    assert set(ALLOCATING_OR_PROBE) <= set(SURVIVING)


@pytest.mark.parametrize("key", RETIRED)
def test_retired_key_is_an_unknown_key(ctx, key):
    from qn_amd import engine
    for value in (0.0, 1.0):
        with pytest.raises(engine.EngineError) as e:
            ctx.debug_set(key, value)
        assert e.value.status == engine.QN_ERR_INVALID_ARG


def test_every_surviving_key_is_accepted(ctx):
    for key, default in SURVIVING.items():
        ctx.debug_set(key, default)


def register(engine, knobs):
    src, tgt, _ = synth.make_pair(7, 700, extent=25.0)
    ctx = engine.Context(1024)
    for k, v in knobs.items():
        ctx.debug_set(k, v)
    g = engine.NanoGICP(ctx)
    g.setInputSource(src); g.calculateSourceCovariances(); g.setInputTarget(tgt); g.calculateTargetCovariances()
    r = g.align()
    out = (np.array(r.T).tobytes(), np.array(r.T64).tobytes(), np.float64(r.fitness).tobytes(), np.float64(g.getFitnessScore()).tobytes(), r.iterations, r.converged)
    ctx.close()
    return out


def test_defaults_set_by_key_change_nothing():
    from qn_amd import engine
    untouched = register(engine, {})
    defaults = register(engine, {k: v for k, v in SURVIVING.items() if k not in ALLOCATING_OR_PROBE})
    assert untouched[4] > 0 and np.isfinite(np.frombuffer(untouched[2], dtype=np.float64)).all()      # (a registration that ran, not two identical failures)
    assert untouched == defaults
