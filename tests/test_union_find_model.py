"""Every interleaving of the two linkers of csrc/qn_union_find.cuh on tiny forests, by the step machines of tests/union_find_model.py (one step = one atomic
memory operation, sequentially consistent per word).  No GPU: a GPU run samples the schedules the hardware happens to produce, this search takes them all,
at the sizes below and no further.

At every state parent[x] <= x and parent[x] lies in x's final component; the state graph has no cycle, so every schedule ends; at every final state the
root of every node is the smallest node of its component.  Configurations (every multiset of lane programs):
  3 lanes x 1 edge x 5 nodes from the identity and 2 lanes x 1 edge x 5 nodes from every forest with parent0[x] <= x, the edge any (a, b) with a != b;
  2 lanes x 2 edges in sequence x 4 nodes from the identity, the edges a < b only (both ways round it is 1.2 million states and 10 s a linker, for an order
  of the two finds that the one-edge configurations already vary).
The state counts and times are printed (about 1.6e5, 5.5e5 and 8e4 states; 2 s, 6 s and under 1 s).  The search must also be able to fail: two
deliberately wrong linkers - a min link that returns after any store instead of going on with the parent it displaced, a swap link that gives up after a
failed swap - must raise, at 2 lanes x 4 nodes.  A plain-store halving in place of the fetch-min passes too at these sizes: nothing here says the halving
has to be an atomic min."""
import time
import pytest
import union_find_model as uf

CONFIGS = {"3 lanes x 5 nodes, identity": dict(n=5, lanes=3), "2 lanes x 5 nodes, every forest": dict(n=5, lanes=2, all_forests=True),
           "2 lanes x 2 edges x 4 nodes, identity": dict(n=4, lanes=2, edges_per_lane=2, ordered=False)}


@pytest.mark.parametrize("config", list(CONFIGS))
@pytest.mark.parametrize("link", [uf.SWAP, uf.MIN])
def test_every_interleaving_ends_at_the_component_minima(link, config):
    t0 = time.perf_counter()
    states = uf.explore_all(link, uf.HALVE_MIN, **CONFIGS[config])
    print("%s link, %s: %d states, %.1f s" % (link, config, states, time.perf_counter() - t0))
    assert states > 10000


@pytest.mark.parametrize("link", [uf.SWAP, uf.MIN])
def test_a_plain_store_halving_passes_too(link):
    assert uf.explore_all(link, uf.HALVE_STORE, n=4, lanes=2, all_forests=True) > 1000


@pytest.mark.parametrize("link", [uf.MIN_RETURNS_AFTER_A_STORE, uf.SWAP_GIVES_UP])
def test_the_search_sees_a_wrong_linker(link):
    with pytest.raises(uf.ModelError):
        uf.explore_all(link, uf.HALVE_MIN, n=4, lanes=2, all_forests=True)


def test_the_step_machine_runs_one_lane_like_a_serial_union_find():
    """one lane alone is the serial algorithm: from a chain 3 -> 2 -> 1 -> 0 and a root 4, unite(3, 4) halves 3's path and hangs 4 under 0"""
    for link in (uf.SWAP, uf.MIN):
        parent, lane = (0, 0, 1, 2, 4), uf.start([(3, 4)])
        steps = 0
        while lane[2]:
            parent, lane = uf.step(link, uf.HALVE_MIN, parent, lane)
            steps += 1
        assert parent == (0, 0, 1, 1, 0) and steps == 7, (link, parent, steps)
    assert uf.components((0, 0, 2, 3, 3), [[(1, 2)], [(3, 3)]]) == (0, 0, 0, 3, 3)
    assert len(uf.forests(5)) == 120 and uf.forests(5)[0] == (0, 1, 2, 3, 4) and len(uf.programs(4, 2, ordered=False)) == 36 and len(uf.programs(5, 1)) == 20
