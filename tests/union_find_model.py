"""The lock-free union-find of csrc/qn_union_find.cuh restated as step machines, and a search over every interleaving of a few lanes on a tiny forest.

Mirrors csrc/qn_union_find.cuh (uf_find, uf_unite, uf_unite_min): whoever changes one changes the other.

One step is one atomic memory operation of one lane: in a trip of uf_find the load of parent[x], the load of parent[p] and the fetch-min of the halving; in a
link the compare-and-swap (uf_unite) or the fetch-min (uf_unite_min).  What a lane does between two memory operations - compares, the choice of hi and lo,
going on to its next edge - belongs to the step before.  A step reads and writes the one array every lane sees: steps are sequentially consistent per word.
That is the whole memory model here.  It says nothing about relaxed reordering of one lane's operations on different words, and nothing for more lanes or
nodes than a search was run with.

A lane is the tuple (edges, ei, pc, a, b, x, y): its edges, the index of the one it is working on, where it stands, and its registers (the unused ones 0):
  pc 1 / 4   find of a / of b: about to load parent[x]
  pc 2 / 5   about to load parent[y], y = the parent just read
  pc 3 / 6   about to halve: parent[x] = min(parent[x], y), y = the grandparent; then on from x = y
  pc 7       both roots found, a != b: about to link hi = max(a, b) under lo = min(a, b)
  pc 0       done, ei == len(edges)
A state is (comp, parent, lanes): comp[x] = the smallest node of x's component in the starting forest plus all edges of all lanes - where every schedule
has to end - and the lanes sorted, since they are interchangeable.

explore() walks the state graph depth first and raises ModelError when
  a state has parent[x] > x, or parent[x] outside x's final component (the invariant qn_union_find.cuh claims for the min link; the swap link's is stronger),
  the graph has a cycle (a schedule that never ends),
  a final state - every lane done - has a node whose chain does not end at the smallest node of its component.
LINKS has the two linkers and two deliberately wrong ones, which the test must see fail; HALVINGS the header's fetch-min and a plain store."""
from itertools import combinations, combinations_with_replacement, permutations, product

SWAP, MIN, MIN_RETURNS_AFTER_A_STORE, SWAP_GIVES_UP = "swap", "min", "min returns after a store", "swap gives up"
LINKS = (SWAP, MIN, MIN_RETURNS_AFTER_A_STORE, SWAP_GIVES_UP)
HALVE_MIN, HALVE_STORE = "fetch-min", "store"
HALVINGS = (HALVE_MIN, HALVE_STORE)


class ModelError(AssertionError):
    pass


def _next_edge(edges, ei):
    ei += 1
    if ei == len(edges):
        return (edges, ei, 0, 0, 0, 0, 0)
    a, b = edges[ei]
    return (edges, ei, 1, 0, b, a, 0)


def start(edges):
    """the lane that will run uf_unite over `edges` in turn"""
    return _next_edge(tuple(edges), -1)


def _found_b(edges, ei, a, b):
    return _next_edge(edges, ei) if a == b else (edges, ei, 7, a, b, 0, 0)


def step(link, halving, parent, lane):
    """one memory operation of `lane` on `parent` (a tuple) -> (parent, lane)"""
    edges, ei, pc, a, b, x, y = lane
    if pc == 1:                                                                  # uf_find(a): p = load(parent + x)
        p = parent[x]
        return parent, ((edges, ei, 4, x, 0, b, 0) if p == x else (edges, ei, 2, 0, b, x, p))
    if pc == 2:                                                                  # g = load(parent + p)
        g = parent[y]
        return parent, ((edges, ei, 4, y, 0, b, 0) if g == y else (edges, ei, 3, 0, b, x, g))
    if pc == 4:                                                                  # uf_find(b)
        p = parent[x]
        return parent, (_found_b(edges, ei, a, x) if p == x else (edges, ei, 5, a, 0, x, p))
    if pc == 5:
        g = parent[y]
        return parent, (_found_b(edges, ei, a, y) if g == y else (edges, ei, 6, a, 0, x, g))
    if pc == 3 or pc == 6:                                                       # path halving, then x = g
        if halving == HALVE_STORE or y < parent[x]:
            parent = parent[:x] + (y,) + parent[x + 1:]
        return parent, (edges, ei, pc - 2, a, b, y, 0)
    assert pc == 7
    hi, lo = (a, b) if a > b else (b, a)
    seen = parent[hi]
    if link == SWAP or link == SWAP_GIVES_UP:                                    # compare_exchange(parent + hi, hi, lo)
        if seen == hi:
            return parent[:hi] + (lo,) + parent[hi + 1:], _next_edge(edges, ei)
        return parent, (_next_edge(edges, ei) if link == SWAP_GIVES_UP else (edges, ei, 1, 0, lo, seen, 0))
    stored = lo < seen                                                           # fetch_min(parent + hi, lo)
    if stored:
        parent = parent[:hi] + (lo,) + parent[hi + 1:]
    if seen == hi or (link == MIN_RETURNS_AFTER_A_STORE and stored):
        return parent, _next_edge(edges, ei)
    return parent, (edges, ei, 1, 0, lo, seen, 0)                                # on with (seen, lo): hi's parent of then


def components(forest, edge_lists):
    """-> comp, comp[x] = the smallest node of x's component in the forest plus the edges"""
    comp = list(range(len(forest)))

    def root(x):
        while comp[x] != x:
            x = comp[x]
        return x
    for a, b in [(x, p) for x, p in enumerate(forest)] + [e for edges in edge_lists for e in edges]:
        ra, rb = root(a), root(b)
        if ra != rb:
            comp[max(ra, rb)] = min(ra, rb)
    return tuple(root(x) for x in range(len(forest)))


def _check_parent(comp, parent):
    for x, p in enumerate(parent):
        if p > x:
            raise ModelError("parent[%d] = %d > %d: %r" % (x, p, x, (parent,)))
        if comp[p] != comp[x]:
            raise ModelError("parent[%d] = %d lies outside the component of %d: %r, components %r" % (x, p, x, parent, comp))


def _check_final(comp, parent):
    for x in range(len(parent)):
        r = x
        while parent[r] != r:
            r = parent[r]
        if r != comp[x]:
            raise ModelError("every lane is done and the root of %d is %d, not %d: %r" % (x, r, comp[x], (parent,)))


def explore(link, halving, forest, edge_lists, seen=None):
    """every interleaving of the lanes that run uf_unite over edge_lists[k] in turn, from `forest`.  seen: the states finished by earlier calls (shared between
    the starts of one configuration, which meet in many states).  -> the number of states new to this call"""
    seen = {} if seen is None else seen
    forest = tuple(forest)
    comp = components(forest, edge_lists)
    first = (comp, forest, tuple(sorted(start(e) for e in edge_lists)))
    if first in seen:
        return 0
    before = len(seen)
    checked = set()

    def successors(state):
        _, parent, lanes = state
        if parent not in checked:
            _check_parent(comp, parent)
            checked.add(parent)
        out = []
        for k, lane in enumerate(lanes):
            if lane[2] == 0 or (k and lane == lanes[k - 1]):                     # done, or the twin of the lane before: the same successor
                continue
            p2, l2 = step(link, halving, parent, lane)
            out.append((comp, p2, tuple(sorted(lanes[:k] + (l2,) + lanes[k + 1:]))))
        if not out:
            _check_final(comp, parent)
        return out

    seen[first] = 1                                                              # 1: on the stack, 2: finished
    stack = [(first, iter(successors(first)))]
    while stack:
        state, it = stack[-1]
        for nxt in it:
            mark = seen.get(nxt)
            if mark is None:
                seen[nxt] = 1
                stack.append((nxt, iter(successors(nxt))))
                break
            if mark == 1:
                raise ModelError("a schedule that never ends: the state graph has a cycle through %r" % (nxt[1:],))
        else:
            seen[state] = 2
            stack.pop()
    return len(seen) - before


def forests(n):
    """every starting forest with parent0[x] <= x on n nodes, the identity first"""
    return sorted(product(*[range(x + 1) for x in range(n)]), key=lambda f: f != tuple(range(n)))


def programs(n, edges_per_lane, ordered=True):
    """every list of edges_per_lane edges a lane may be given on n nodes, in every order and with repeats: the edges (a, b), a != b, both ways round (the
    order decides which end's find runs first), or with ordered = False only a < b"""
    pairs = list(permutations(range(n), 2)) if ordered else list(combinations(range(n), 2))
    return list(product(pairs, repeat=edges_per_lane))


def explore_all(link, halving, n, lanes, edges_per_lane=1, all_forests=False, ordered=True):
    """explore() for every multiset of `lanes` programs on n nodes, from the identity or from every forest -> the number of states"""
    seen = {}
    starts = forests(n) if all_forests else [tuple(range(n))]
    for forest in starts:
        for lists in combinations_with_replacement(programs(n, edges_per_lane, ordered), lanes):
            explore(link, halving, forest, lists, seen)
    return len(seen)
