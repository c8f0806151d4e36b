"""tools/replay.py --max-see-through: the free-space veto on the loop replay.  Off (the default) a run is what it is without the option; on, a run without
false loops is unchanged and every attempt carries both directions' see-through fractions; a pair fed a deliberately wrong transform is refused.
Uniform stream, 40 keyframes, seed 11, Scan Context + relative verification on the oracle backend: the run closes (20, 0) and rejects (30, 9) and (35, 12) on
their scores.  Fractions there (query in candidate, candidate in query; 32 x 360 image over +-60 degrees): (20, 0) 0.0115 / 0.0159; (30, 9) 0.0626 / 0.1123;
(35, 12) 0.1119 / 0.1473; (20, 0) turned by 180 degrees: see test_a_wrong_transform_is_refused's output.  The bound used below, 0.05, lies between the
accepted pair's and the rejected pairs' figures of that probe; the tests assert decisions, not the figures.
Under -m gpu: the GPU replay takes the same decisions as the oracle replay with the gate on."""
import math
import os
import sys
import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
KW = dict(n_kf=40, seed=11, verbose=False, backend="oracle", detector="scancontext", verify="relative")


def test_the_gate_leaves_a_run_without_false_loops_unchanged():
    import replay
    off = replay.run(**KW)
    assert [(q, c) for q, c, _ in off["loop_list"]] == [(20, 0)] and off["attempts"] == 3 and "see_through" not in off
    same = replay.run(max_see_through=None, range_params=None, **KW)
    assert same["loop_list"] == off["loop_list"] and all(np.array_equal(p, q) for p, q in zip(same["poses"], off["poses"]))
    on = replay.run(max_see_through=0.05, **KW)
    assert on["loop_list"] == off["loop_list"] and all(np.array_equal(p, q) for p, q in zip(on["poses"], off["poses"]))
    assert [(o["query"], o["cand"], o["valid"], o["accepted"]) for o in on["see_through"]] == [(20, 0, True, True), (30, 9, False, False), (35, 12, False, False)]
    for o in on["see_through"]:
        print(o)
        assert 0.0 <= o["q_in_c"] <= 1.0 and 0.0 <= o["c_in_q"] <= 1.0 and min(o["observed"]) > 1000
    ok = on["see_through"][0]
    assert all(max(o["q_in_c"], o["c_in_q"]) > max(ok["q_in_c"], ok["c_in_q"]) for o in on["see_through"][1:])
    none = replay.run(max_see_through=0.0, **KW)                    # a bound nothing meets: the same attempts, no loop
    assert none["loop_list"] == [] and none["see_through"][0]["valid"] and not none["see_through"][0]["accepted"]


def test_a_wrong_transform_is_refused(monkeypatch):
    """the verification of (20, 0) is made to answer `valid` with its transform turned by 180 degrees: without the gate the false loop goes into the graph,
    with it the pair is dropped"""
    import replay
    real = replay._oracle_relative

    def wrong(orc, scans, poses, k, c, *a, **kw):
        r = real(orc, scans, poses, k, c, *a, **kw)
        if (k, c) == (20, 0):
            Rz = np.eye(4); Rz[:2, :2] = [[-1.0, 0.0], [0.0, -1.0]]
            r = dict(r, T=Rz @ r["T"], valid=True)
        return r

    monkeypatch.setattr(replay, "_oracle_relative", wrong)
    off = replay.run(**KW)
    assert (20, 0) in [(q, c) for q, c, _ in off["loop_list"]]
    on = replay.run(max_see_through=0.05, **KW)
    print(on["see_through"])
    o = on["see_through"][0]
    assert (20, 0) not in [(q, c) for q, c, _ in on["loop_list"]] and (o["query"], o["cand"], o["valid"], o["accepted"]) == (20, 0, True, False)
    assert max(o["q_in_c"], o["c_in_q"]) > 0.05


def test_the_option_is_checked():
    import replay
    for bad in (dict(max_see_through=-0.1), dict(max_see_through=float("nan"))):
        with pytest.raises(ValueError):
            replay.run(**dict(KW, n_kf=4, **bad))
    with pytest.raises(ValueError):
        replay.run(n_kf=4, verbose=False, backend="oracle", max_see_through=0.05)           # the reference-style check has no sensor-frame transform


@pytest.mark.gpu
@pytest.mark.parametrize("sensor", ["uniform", "spinning"])
def test_gpu_replay_equals_the_oracle_replay_with_the_gate_on(sensor):
    import replay
    kw = dict(KW, sensor=sensor, max_see_through=0.05)
    if sensor == "spinning":
        kw.update(n_kf=70, seed=7, yaw_bias=0.02)
    a = replay.run(**dict(kw, backend="gpu"))
    b = replay.run(**kw)
    assert [(k, c) for k, c, _ in a["loop_list"]] == [(k, c) for k, c, _ in b["loop_list"]] and a["attempts"] == b["attempts"]
    assert len(a["see_through"]) == len(b["see_through"]) > 0
    for x, y in zip(a["see_through"], b["see_through"]):
        print(sensor, x, y)
        assert (x["query"], x["cand"], x["valid"], x["accepted"]) == (y["query"], y["cand"], y["valid"], y["accepted"])
        if y["valid"]:      # the two registrations agree to 1e-4 where they converge: a handful of points may change class
            assert abs(x["q_in_c"] - y["q_in_c"]) < 5e-3 and abs(x["c_in_q"] - y["c_in_q"]) < 5e-3
    d = max(np.linalg.norm(p[:3, 3] - q[:3, 3]) for p, q in zip(a["poses"], b["poses"]))
    assert d < 1e-3, d
