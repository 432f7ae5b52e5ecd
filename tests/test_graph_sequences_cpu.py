"""The committed sequences of tests/graph_model.py through the model ALONE (no device): the inputs of
tests/test_graph_sequences_gpu.py are not degenerate.  SEQUENCES holds 10 (k, seed) pairs, the smallest set a greedy cover of the
conditions below found among seeds 0..59 of every k: 2 at k = 21, 2 at 31 (one key word), 3 at 35, 3 at 64 (two words, the tagged
table).  Each is make_input(seed, k) = pairs_ref.make_pairs(seed, k, err=0.004) plus two planted haplotype SNPs, counts below 2
dropped, and STEPS = 8 operations drawn by random.Random(seed).

Asserted here:
  * every operation is EFFECTIVE (it removes or merges an edge, adds a node, or swaps the handle) at a position >= 2 of some
    sequence, right behind an effective step; and, a condition of this file's own, at every k somewhere;
  * each ordered pair / triple of ORDERS occurs, nothing in it skipped, its last step effective;
  * at most 1 step in 8 overall is skipped (a retain that would have to break a tie among node copies; an add node without a
    candidate), and the file counts them;
  * the content is strand-closed after every step up to the first one at which the REFERENCE gives strand symmetry up.

Where this departs from a plain reading of those conditions, because the reference leaves no choice:
  * pairs+split -> reload -> simplify occurs, but its simplify cannot be effective: the oracle's split_by_support ends with
    simplifyGraph (GraphSimplifier.scala:318), so the step's device side does too and nothing is left to merge.  Asserted as it
    is: the triple occurs, and no simplify behind a pairs+split (a reload between or not) is ever effective.
  * strand symmetry ends not only with pairs+split and add node.  removeBubbles keeps the first of two parallel edges in each
    node's own out-edge order, so the two strands of a bubble may keep different arms; and a strand-closed graph without node
    copies is two mirror-image sets of components, so its retainLargest always breaks a tie (by the stated rule, "the one holding
    the smallest k-mer": components_ref and the oracle agree, asserted in the model) and keeps one strand.  Such a retain is
    run, not skipped: skipping every tie would leave retain without work before the first split.  Closure is asserted up to the
    first effective one of these four, and it is asserted that nothing else ever breaks it.
"""
import pytest

import graph_model as GM
import tips_ref as T

ORDERS = [("simplify", "clip"), ("simplify", "pop"), ("retain", "simplify"), ("retain", "reload", "clip"), ("remove_id", "retain"),
          ("split", "retain"), ("split", "reload", "simplify"), ("clip", "split"), ("reload", "addnode"), ("addnode", "split")]
NEVER_EFFECTIVE = ("split", "reload", "simplify")
ONE_STRAND_AFTER = ("split", "addnode", "bubbles", "retain")


@pytest.fixture(scope="module")
def runs():
    """every committed sequence, once -> {(k, seed): [(operation, effective, skipped, strand-closed or None once it need not be)]}"""
    out = {}
    for k, seed in GM.SEQUENCES:
        m = GM.GraphModel(k, seed)
        assert T.strand_closed(m.content()[1]) and not m.has_copies()
        reads_at, symmetric, rows = GM.observer_steps(seed), True, []
        for step in range(GM.STEPS):
            op = m.draw()
            res = m.step(op)
            if op in ONE_STRAND_AFTER and res["effective"]:
                symmetric = False
            rows.append((op, res["effective"], bool(res.get("skip")), T.strand_closed(m.content()[1]) if symmetric else None))
            # what the device's observers will be held to can be computed in every state the sequence reaches
            nodes, edges = m.content()
            assert m.expect_counts() == (len(nodes), len(edges), sum(len(e[2]) for e in edges))
            assert sorted(m.expect_degrees()) == sorted(set(nodes)) == sorted(m.expect_out_bases())
            assert sum(n for n, _ln in m.components()[0]) == len(nodes)
            if step in reads_at:
                sup, st = m.expect_thread(m.reads[:300])
                assert st["records"] == 300 and st["inner_windows"] > 0
                assert m.expect_pair_distances(200)[1]["orientations"] == 400
        assert [r[:3] for r in rows] == m.history
        out[(k, seed)] = rows
    return out


def test_the_committed_list():
    assert len(GM.SEQUENCES) == len(set(GM.SEQUENCES)) == 10
    assert {k for k, _s in GM.SEQUENCES} == {21, 31, 35, 64}
    assert GM.SMALL_GRID in GM.SEQUENCES


def test_every_operation_is_effective_behind_an_effective_step(runs):
    seen = {op: [] for op in GM.OPS}
    for key, rows in runs.items():
        for i, (op, effective, _skipped, _closed) in enumerate(rows):
            if i >= 2 and effective and rows[i - 1][1]:
                seen[op].append(key + (i,))
    assert all(seen.values()), [op for op, at in seen.items() if not at]


def test_every_operation_is_effective_at_every_k(runs):
    seen = {(k, op) for (k, _seed), rows in runs.items() for op, effective, _s, _c in rows if effective}
    assert seen == {(k, op) for k in (21, 31, 35, 64) for op in GM.OPS}


def occurrences(runs, order):
    """[(k, seed, position of the last step, its effectiveness)] of the unskipped occurrences of `order` as consecutive steps"""
    n, out = len(order), []
    for key, rows in runs.items():
        for i in range(len(rows) - n + 1):
            w = rows[i:i + n]
            if tuple(r[0] for r in w) == order and not any(r[2] for r in w):
                out.append(key + (i + n - 1, w[-1][1], w[0][1]))
    return out


@pytest.mark.parametrize("order", ORDERS, ids=["->".join(o) for o in ORDERS])
def test_orders_the_tools_never_use(runs, order):
    found = occurrences(runs, order)
    if order == NEVER_EFFECTIVE:
        assert found and not any(f[3] for f in found)
    elif order == ("addnode", "split"):                       # the index was built by the nodeId observer before the add node,
        assert any(f[3] and f[4] for f in found)              # patched by it, and is looked at again after the split
    else:
        assert any(f[3] for f in found)


def test_a_simplify_behind_a_split_has_nothing_left_to_do(runs):
    for rows in runs.values():
        for i, (op, effective, _s, _c) in enumerate(rows):
            j = i - 1
            while j >= 0 and rows[j][0] == "reload":
                j -= 1
            if op == "simplify" and j >= 0 and rows[j][0] == "split":
                assert not effective


def test_few_steps_are_skipped(runs):
    skipped = sum(1 for rows in runs.values() for r in rows if r[2])
    total = sum(len(rows) for rows in runs.values())
    assert total == GM.STEPS * len(GM.SEQUENCES) and 8 * skipped <= total, (skipped, total)


def test_strand_closed_until_the_reference_gives_it_up(runs):
    checked = 0
    for key, rows in runs.items():
        for i, (op, _e, _s, closed) in enumerate(rows):
            if closed is not None:
                assert closed, key + (i, op)
                checked += 1
    assert checked >= len(GM.SEQUENCES)
