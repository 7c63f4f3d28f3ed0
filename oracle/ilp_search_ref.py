"""CPU restatement of the device solver's branch and bound (TEST INFRASTRUCTURE ONLY).

The search as the comments of rgc_ilp.hip describe it (header, k_ilp_small, k_ilp_wave), per
conflict component:
  * members ordered by (weight descending, column ascending);
  * depth first: include the heaviest remaining candidate, then exclude it;
  * pruned by the greedy clique cover by boxes: heaviest candidate first, a candidate with one
    of its boxes already open is covered, otherwise it opens its box with the most columns
    (ties: the first in the column's row order) and adds its weight; a node is cut when
    value + bound <= incumbent;
  * the incumbent is replaced only by a strictly greater value;
  * one node per loop trip (leaves, cut nodes and the final unwinding trip included).

Neither the wave solver's Lagrangian bound nor its seeded incumbent is modelled.  Both only cut
nodes that cannot hold a packing strictly better than the incumbent (the seed enters a hair
below its value), and the 1e-4 early stop begins at 65,536 nodes, above the default budget: so
the node count here is an upper bound on the device's, and whenever the device finishes its x
is the x found here, the first optimal leaf in search order.

Weights are f32 values summed in f64 (exact), as on the device.
"""
from __future__ import annotations

import numpy as np
from scipy.sparse import csc_matrix

from . import ilp_ref

DEFAULT_NODES = 1 << 14   # include/repic_gc.h RGC_ILP_DEFAULT_NODES
SMALL_MAX = 64            # k_ilp_small: one thread per component
BIG_MAX = 4096            # k_ilp_wave: one wavefront per component; larger ones are not searched


def node_budget(n, node_limit=DEFAULT_NODES):
    """Nodes the device grants a component of n columns: node_limit up to 1024 columns
    (W = ceil(n / 64) <= 16 words per bitset), node_limit * 16 // W above."""
    W = (n + 63) // 64
    return node_limit if W <= 16 else node_limit * 16 // W


def search_component(col_rows, w, budget):
    """Branch and bound over one conflict component.  col_rows[i]: the rows of column i in the
    order the solver is given them; w[i]: its weight.  Returns (x uint8 in the given column
    order, objective, nodes, proven)."""
    n = len(col_rows)
    w = np.asarray(w, np.float64)
    order = sorted(range(n), key=lambda i: (-w[i], i))
    wl = [float(w[i]) for i in order]
    row_cols = {}   # row -> bitset of the members (local numbering) on it
    for li, i in enumerate(order):
        for r in col_rows[i]:
            row_cols[r] = row_cols.get(r, 0) | (1 << li)
    adj, opener = [], []
    for li, i in enumerate(order):
        a, best_deg, best_row = 0, -1, None
        for r in col_rows[i]:
            a |= row_cols[r]
            deg = bin(row_cols[r]).count("1")
            if deg > best_deg:
                best_deg, best_row = deg, r
        adj.append(a & ~(1 << li))
        # opening a box covers every candidate on it, the opener included
        opener.append(row_cols[best_row])

    def bound(P):
        # a candidate still in P has none of its boxes open: each opened box removed its columns
        s = 0.0
        while P:
            i = (P & -P).bit_length() - 1
            s += wl[i]
            P &= ~opener[i]
        return s

    best, cur, best_set, chosen = -1.0, 0.0, 0, 0
    P = (1 << n) - 1
    stack = []   # frames [P, cur, j, on include branch]
    nodes, proven = 0, True
    while True:
        back = False
        nodes += 1
        if nodes > budget:
            proven = False
            break
        if P == 0:
            if cur > best:
                best, best_set = cur, chosen
            back = True
        elif cur + bound(P) <= best:
            back = True
        else:
            j = (P & -P).bit_length() - 1
            stack.append([P, cur, j, True])
            P &= ~adj[j] & ~(1 << j)
            cur += wl[j]
            chosen |= 1 << j
        if back:
            found = False
            while stack:
                fr = stack[-1]
                if fr[3]:
                    fr[3] = False
                    j = fr[2]
                    P = fr[0] & ~(1 << j)
                    cur = fr[1]
                    chosen &= (1 << j) - 1
                    found = True
                    break
                stack.pop()
            if not found:
                break
    x = np.zeros(n, np.uint8)
    for li, i in enumerate(order):
        x[i] = (best_set >> li) & 1
    return x, float(sum(wl[li] for li in range(n) if (best_set >> li) & 1)), nodes, proven


def solve(A, w, node_limit=DEFAULT_NODES):
    """The documented search on every conflict component of the model, each under the device's
    budget for its size.  Returns (x, objective, nodes, proven): nodes is the largest count of
    one component; proven is False if a component ran out of budget or has more than BIG_MAX
    columns (the device does not search those; their x stays 0 here).  A component of one
    column takes it iff its weight is positive."""
    A = csc_matrix(A)
    w = np.asarray(w, np.float64)
    x = np.zeros(A.shape[1], np.uint8)
    if A.shape[1] == 0:
        return x, 0.0, 0, True
    ncomp, lab = ilp_ref.components(A)
    mem = [[] for _ in range(ncomp)]
    for j, c in enumerate(lab.tolist()):
        mem[c].append(j)
    nodes, proven = 0, True
    for cols in mem:
        if len(cols) == 1:
            x[cols[0]] = 1 if w[cols[0]] > 0.0 else 0
            continue
        if len(cols) > BIG_MAX:
            proven = False
            continue
        rows = [A.indices[A.indptr[j]:A.indptr[j + 1]].tolist() for j in cols]
        xc, _, nd, pr = search_component(rows, w[cols], node_budget(len(cols), node_limit))
        x[cols] = xc
        nodes = max(nodes, nd)
        proven = proven and pr
    return x, float(np.sum(w[x == 1])), nodes, proven
