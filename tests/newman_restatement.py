"""Test-side restatement of the Girvan-Newman partition (csrc/newman.hip, cgmap.partition_newman; reference get_partition /
parition2mapping, CoarseGrainingVAE/datasets.py:363-385), written from the algorithm and taken from no package:

    betweenness of edge e = sum over ALL sources s of Brandes' dependency of s on e          (fp64; path counts are
                            integers held in fp64, exact far beyond these sizes)
    removal               = among the live edges within a relative 1e-9 of the maximum, the lowest (min(u,v), max(u,v))
    stop                  = when the graph has n_cgs connected components
    bead k                = the component with the k-th smallest lowest atom index

Also here: the molecule-like test graphs both test files use, and the networkx runs they are compared with."""
import functools
import itertools
from collections import deque

import numpy as np

TIE = 1e-9
# (n_atoms, ring-closing edges, n_cgs), each with seeds 0..3: twenty graphs
SETTINGS = ((22, 0, 3), (22, 2, 3), (40, 3, 6), (64, 4, 8), (166, 8, 6))
SEEDS = (0, 1, 2, 3)
CASES = tuple((n, rings, k, seed) for n, rings, k in SETTINGS for seed in SEEDS)


def case_id(case):
    return "n{}_r{}_k{}_s{}".format(*case)


def sorted_edges(edges):
    e = np.sort(np.asarray(edges, dtype=np.int64).reshape(-1, 2), axis=1)
    return np.unique(e, axis=0).reshape(-1, 2)


def _adjacency(n, edges, alive):
    adj = [[] for _ in range(n)]
    for e, (u, v) in enumerate(edges):
        if alive[e]:
            adj[u].append((v, e))
            adj[v].append((u, e))
    return adj


def edge_betweenness(n, edges, alive=None):
    """fp64 [m]: the sum over all sources of the source's dependency on each edge (every unordered pair counts twice)."""
    edges = [tuple(int(x) for x in e) for e in edges]
    alive = [1] * len(edges) if alive is None else list(alive)
    adj = _adjacency(n, edges, alive)
    bet = [0.0] * len(edges)
    for s in range(n):
        level, sigma, order = [-1] * n, [0.0] * n, []
        level[s], sigma[s] = 0, 1.0
        queue = deque([s])
        while queue:
            v = queue.popleft()
            order.append(v)
            for w, _ in adj[v]:
                if level[w] < 0:
                    level[w] = level[v] + 1
                    queue.append(w)
                if level[w] == level[v] + 1:
                    sigma[w] += sigma[v]
        delta = [0.0] * n
        for w in reversed(order):
            for v, e in adj[w]:
                if level[v] == level[w] - 1:
                    c = sigma[v] / sigma[w] * (1.0 + delta[w])
                    delta[v] += c
                    bet[e] += c
    return np.array(bet, dtype=np.float64)


def component_labels(n, edges, alive=None):
    """int64 [n]: the lowest atom index of each atom's component."""
    alive = [1] * len(edges) if alive is None else alive
    adj = _adjacency(n, [tuple(int(x) for x in e) for e in edges], alive)
    label = [-1] * n
    for s in range(n):
        if label[s] >= 0:
            continue
        label[s] = s
        queue = deque([s])
        while queue:
            v = queue.popleft()
            for w, _ in adj[v]:
                if label[w] < 0:
                    label[w] = s
                    queue.append(w)
    return np.array(label, dtype=np.int64)


def choose_edge(bet, edges, alive):
    """The tie rule.  Returns the edge index."""
    live = [e for e in range(len(edges)) if alive[e]]
    top = max(bet[e] for e in live)
    near = [e for e in live if bet[e] >= top - TIE * top]
    return min(near, key=lambda e: (min(edges[e]), max(edges[e])))


def partition(n, edges, n_cgs):
    """(mapping int64 [n], removed edges [(u, v), ...] in order, exact-or-near ties met)."""
    edges = [tuple(int(x) for x in e) for e in edges]
    alive = [1] * len(edges)
    labels = component_labels(n, edges, alive)
    removed, ties = [], 0
    while len(set(labels.tolist())) < n_cgs:
        bet = edge_betweenness(n, edges, alive)
        e = choose_edge(bet, edges, alive)
        top = max(bet[i] for i in range(len(edges)) if alive[i])
        ties += sum(1 for i in range(len(edges)) if alive[i] and bet[i] >= top - TIE * top) > 1
        alive[e] = 0
        removed.append(edges[e])
        labels = component_labels(n, edges, alive)
    return np.unique(labels, return_inverse=True)[1].astype(np.int64), removed, ties


def as_sets(mapping):
    m = np.asarray(mapping).tolist()
    return {frozenset(i for i, b in enumerate(m) if b == k) for k in set(m)}


# ------------------------------------------------------------------ the test graphs
def molecule_graph(n, rings, seed):
    """A molecule-like graph: a random tree with degree <= 4 grown atom by atom (mostly along the chain, sometimes a
    branch), plus ``rings`` edges that close rings of five or six atoms.  Edges int64 [m,2], u < v, sorted."""
    rng = np.random.default_rng([int(seed), int(n), int(rings)])
    deg = np.zeros(n, dtype=np.int64)
    edges = []
    for v in range(1, n):
        recent = [u for u in range(max(0, v - 4), v) if deg[u] < 4]
        pool = recent if recent and rng.random() < 0.85 else [u for u in range(v) if deg[u] < 4]
        u = int(pool[rng.integers(len(pool))])
        edges.append((u, v))
        deg[u] += 1
        deg[v] += 1
    closed = 0
    for _ in range(1000):
        if closed == rings:
            break
        adj = _adjacency(n, edges, [1] * len(edges))
        a = int(rng.integers(n))
        if deg[a] >= 4:
            continue
        dist = {a: 0}
        queue = deque([a])
        while queue:
            x = queue.popleft()
            if dist[x] == 5:
                continue
            for y, _ in adj[x]:
                if y not in dist:
                    dist[y] = dist[x] + 1
                    queue.append(y)
        ends = sorted(b for b, d in dist.items() if d in (4, 5) and deg[b] < 4)
        if not ends:
            continue
        b = int(ends[rng.integers(len(ends))])
        edges.append((min(a, b), max(a, b)))
        deg[a] += 1
        deg[b] += 1
        closed += 1
    assert closed == rings
    return sorted_edges(edges)


@functools.lru_cache(maxsize=None)
def case_graph(case):
    n, rings, _, seed = case
    return molecule_graph(n, rings, seed)


@functools.lru_cache(maxsize=None)
def case_partition(case):
    """The restatement's answer for one of CASES, computed once per process and shared (read only)."""
    n, _, k, _ = case
    return partition(n, case_graph(case), k)


# ------------------------------------------------------------------ networkx (the reference's route)
def networkx_partition(n, edges, n_cgs):
    """get_partition + parition2mapping (datasets.py:363-385) on a graph with nodes added 0..n-1 and edges in sorted order.
    Returns (mapping int64 [n], flagged): ``flagged`` counts removals where another edge lay within a relative 1e-6 of the
    maximum WITHOUT being bitwise equal to it -- there networkx's first-maximum choice is rounding noise."""
    import networkx as nx
    G = nx.Graph()
    G.add_nodes_from(range(n))
    G.add_edges_from((int(u), int(v)) for u, v in edges)
    flagged = [0]

    def most_valuable_edge(g):
        bet = nx.edge_betweenness_centrality(g)
        best = max(bet, key=bet.get)                                   # what girvan_newman does by default
        top = bet[best]
        if any(v != top and abs(v - top) <= 1e-6 * top for v in bet.values()):
            flagged[0] += 1
        return best
    communities = None
    for communities in itertools.islice(nx.community.girvan_newman(G, most_valuable_edge=most_valuable_edge), n_cgs - 1):
        pass
    mapping = np.zeros(n, dtype=np.int64)
    for k, group in enumerate(tuple(sorted(c) for c in communities)):
        for node in group:
            mapping[node] = k
    return mapping, flagged[0]


@functools.lru_cache(maxsize=None)
def case_networkx(case):
    n, _, k, _ = case
    return networkx_partition(n, case_graph(case), k)
