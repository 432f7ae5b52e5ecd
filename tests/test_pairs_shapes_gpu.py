"""Paired-end walks at the shapes they were built for (-m gpu): the reference's range 180..250 (GraphSimplifier.scala:146), every
key width of `k_pair_keys` (k = 31, 34, 47, 55, 62, 63, 64), 100- to 255-base mates, ranges that meet the mates' distance
exactly, an edge longer than the 16 bits a walk state holds of a distance, walks that outgrow the wave's LDS sets on their own,
ragged and degenerate `.bin` streams, and graphs that were edited before they are walked.

Every case compares FIVE quantities with the C oracle's literal restatement (O.Graph.walk_pairs / split_by_support): walked
orientations, bad pairs, the support by content, the (removed, new nodes) of splitBySupport, and the canonical graph after
simplifyGraph.  Before any device call a case asserts, on the oracle's results alone, that its fixture is not vacuous.

`Support.last_walk()` (a test hook) says how many orientations the device kernel handed to the host walker: a result is only
credited to the kernel where it did the walking.

Fixtures: pairs_ref.make_pairs — an 8 kbp genome with 4 planted repeats, 6000 pairs, 0.5 % substitutions, inserts drawn so that
insert - k (the distance a walk measures between the mates' first k-mers) lies inside the range under test."""
import random

import numpy as np
import pytest

from genome_amd import _lib as L
from genome_amd import dna
from genome_amd.dnamap import Context, HipDNAMap
from genome_amd.graph import Support, buildGraph
from oracle import oracle as O
from oracle import pyref as R
from pairs_ref import gpu_canonical, gpu_support_by_content, make_pairs, oracle_canonical, oracle_support_by_content

pytestmark = pytest.mark.gpu

RANGE = (180, 250)                 # the reference's
GLEN, NREP, NPAIRS = 8000, 4, 6000


@pytest.fixture(scope="module")
def ctx():
    c = Context(0)
    yield c
    c.close()


def inserts(k, L, rng=RANGE):
    """insert lengths whose walk distance, insert - k, lies 5 inside `rng`; never shorter than a mate (a uniform stream)"""
    return max(k + rng[0] + 5, L), k + rng[1] - 5


def pairs(seed, k, L, err=0.005, npairs=NPAIRS, ins=None, **kw):
    return make_pairs(seed, k, glen=GLEN, nrep=NREP, L=L, npairs=npairs, ins=ins or inserts(k, L), err=err, **kw)


def cut_at(reads, nrecords):
    """bytes of the first `nrecords` records of reads_to_bin(reads)"""
    return sum(1 + (len(r) + 3) // 4 for r in reads[:nrecords])


def oracle_graph(k, binb, nreads, min_count, edit=False):
    ref = O.PMap(k, 1)
    ref.count_reads(binb, nreads)
    if min_count > 1:
        ref.delete_lt(min_count)
    og = O.Graph(ref)
    if edit:
        og.remove_bubbles(); og.simplify()
    return og


def oracle_round(og, k, binb, npairs, rng, cutoff=3, split=True, errors=True, vacuous_ok=False):
    """One walk -> split -> simplify round of the oracle, with the fixture's non-vacuity asserted on ITS results alone."""
    want = {"graph": oracle_canonical(og)}
    osup = O.Support()
    want["walked"] = og.walk_pairs(osup, binb, npairs, *rng)
    want["bad"] = osup.bad_pairs()
    want["support"] = oracle_support_by_content(og, k, osup)
    want["unique_keys"] = len(want["support"]) == len(osup.items()[0])
    if not vacuous_ok:
        assert len(want["support"]) > 0 and max(want["support"].values()) >= cutoff, "vacuous fixture: no support at the cutoff"
        if errors:
            assert want["bad"] >= 1, "vacuous fixture: errors were injected, yet no pair is bad"
    want["split"] = og.split_by_support(osup, cutoff)        # (the oracle's includes simplifyGraph :318)
    if split and not vacuous_ok:
        assert want["split"][1] > 0, "vacuous fixture: the split makes no node"
    want["after"] = oracle_canonical(og)
    return want


def device_graph(ctx, k, binb, nreads, min_count, edit=False):
    m = HipDNAMap(ctx, k)
    m.count_reads(binb, nreads)
    if min_count > 1:
        m.deleteAll_lt(min_count)
    g = buildGraph(k, m)
    if edit:
        g.removeBubbles(); g.simplifyGraph()
    return m, g


def device_round(ctx, g, k, want, batches, rng, cutoff=3):
    """The same round on the device, compared with `want` after every step.  batches: [(bin bytes, npairs)] into ONE support.
    -> (orientations handed to the walk stage, orientations that went to the host walker), summed over the batches."""
    assert gpu_canonical(g) == want["graph"]
    vm = g.getGraphMap()
    sup = Support(ctx)
    orientations = overflowed = 0
    for b, n in batches:
        g.walkPairs(vm, sup, b, n, *rng)
        o, v = sup.last_walk()
        assert v <= o
        orientations += o; overflowed += v
    npairs_distinct, bad, walked = sup.sizes()
    assert walked == want["walked"]
    assert bad == want["bad"]
    assert walked <= orientations
    got = gpu_support_by_content(g, k, sup)
    assert (len(got) == npairs_distinct) == want["unique_keys"]
    assert got == want["support"]
    assert g.splitBySupport(sup, cutoff) == want["split"]
    g.simplifyGraph()
    assert gpu_canonical(g) == want["after"]
    n, e, ln = g.counts()
    assert (n, e, ln) == (len(want["after"][0]), len(want["after"][1]), sum(len(x[2]) for x in want["after"][1]))
    if want["split"] != (0, 0):                              # the position map of the OLD graph no longer describes this one
        with pytest.raises(L.GkError) as err:
            g.walkPairs(vm, Support(ctx), *batches[0], *rng)
        assert err.value.code == L.GK_E_STATE
    sup.close(); vm.close()
    return orientations, overflowed


# ---- a. the reference's range at every key width -----------------------------------------------------------------------

@pytest.mark.parametrize("k,L", [(31, 150), (34, 150), (34, 100), (47, 150), (55, 150), (62, 150), (63, 150), (64, 150), (64, 255)])
def test_reference_range_at_every_key_width(ctx, k, L):
    """k = 31: one word; 34: `low_mask(2 * (k - 32))` = 4 bits of the high word; 47, 55 (C4), 62, 63 (C5): the two-word table;
    64: the tagged table.  150-base mates (38 payload bytes), 100 and 255 (the byte limit of a `.bin` length).  Two walkPairs
    batches accumulate into one support.  The device must have walked: fewer orientations overflow than were handed over."""
    reads = pairs(100 + k, k, L)
    assert {len(r) for r in reads} == {L}
    binb = dna.reads_to_bin(reads)
    npairs = len(reads) // 2
    want = oracle_round(oracle_graph(k, binb, len(reads), 2), k, binb, npairs, RANGE)
    m, g = device_graph(ctx, k, binb, len(reads), 2)
    half = npairs // 2
    cut = cut_at(reads, 2 * half)
    orientations, overflowed = device_round(ctx, g, k, want, [(binb[:cut], half), (binb[cut:], npairs - half)], RANGE)
    assert orientations == 2 * npairs and overflowed < orientations
    g.close(); m.close()


# ---- b. ranges that meet the mates' distance exactly ---------------------------------------------------------------------

D = 200
EDGE_RANGES = [(D, D), (D - 1, D - 1), (D + 1, D + 1), (0, D), (0, D - 1), (D, 65535), (D + 1, 65535), (0, 0), RANGE]


@pytest.mark.parametrize("k", [55, 21, 64])
def test_range_edges_around_one_fixed_distance(ctx, k):
    """Every insert is D + k long, error-free: a walk measures exactly D between the mates' first k-mers (and `annotate`, which
    adds k, D + k: inside 180..250 at k = 21, where it drops the orientations whose mates share an edge; outside at 55 and 64).
    A range that holds D supports pairs; one that misses D by one supports NONE and every walked orientation is bad — asserted
    on the oracle's results, so the sweep cannot go vacuous — and the library must agree with the oracle at each.  hi = 65535 is
    the largest distance a walk state holds (the walks unroll the repeats' cycles up to it and outgrow the LDS sets: the host
    walker's range edge); there the first 400 pairs are walked, an oracle walk of all 3000 takes a minute.  Error-free input
    collapses to under twenty nodes: the split is compared, not asserted to make nodes."""
    reads = pairs(200 + k, k, 100, err=0.0, npairs=3000, ins=(D + k, D + k))
    binb = dna.reads_to_bin(reads)
    wants = {}
    for rng in EDGE_RANGES:
        n = 400 if rng[1] == 65535 else len(reads) // 2
        wants[rng] = oracle_round(oracle_graph(k, binb, len(reads), 2), k, binb, n, rng, split=False, errors=False, vacuous_ok=True)
    hit, miss = [(D, D), (0, D), RANGE], [(D - 1, D - 1), (D + 1, D + 1), (0, D - 1), (0, 0)]
    for rng in hit:
        assert wants[rng]["support"] == wants[(D, D)]["support"] and sum(wants[rng]["support"].values()) > 100
        assert wants[rng]["bad"] < wants[rng]["walked"]
    for rng in miss:
        assert not wants[rng]["support"] and wants[rng]["bad"] == wants[rng]["walked"] > 0
        assert wants[rng]["split"] != wants[(D, D)]["split"]
    for rng in [(D, 65535), (D + 1, 65535)]:
        assert sum(wants[rng]["support"].values()) > 100 and wants[rng]["walked"] > 0
    for rng in EDGE_RANGES:
        m, g = device_graph(ctx, k, binb, len(reads), 2)
        n = 400 if rng[1] == 65535 else len(reads) // 2
        device_round(ctx, g, k, wants[rng], [(binb, n)], rng)
        g.close(); m.close()
    # the limits of the range itself
    m, g = device_graph(ctx, k, binb, len(reads), 2)
    vm, sup = g.getGraphMap(), Support(ctx)
    for lo, hi in [(0, 65536), (D, 65536), (D + 1, D), (251, 250), (-1, 250)]:
        with pytest.raises(L.GkError) as err:
            g.walkPairs(vm, sup, binb, 10, lo, hi)
        assert err.value.code == L.GK_E_INVALID
    assert sup.sizes() == (0, 0, 0)
    sup.close(); vm.close(); g.close(); m.close()


# ---- c. an edge longer than 65 535 bases ------------------------------------------------------------------------------------

@pytest.mark.parametrize("rng", [RANGE, (0, 65535)])
def test_an_edge_longer_than_a_walk_state_holds(ctx, rng):
    """A clean 90 kbp genome with two planted 300-base repeats near its start, 150-base reads tiled every 25 bases on both
    strands (test_vmap_gpu's CheckGraph fixture): the rest of the genome is ONE unitig of 78 kbp per strand, longer than the 16
    bits in which `walk_one` packs a state's distance, with positions on it beyond 65 535.  Pairs are drawn round the repeats
    (walks that leave and enter the long edges) and deep inside the long unitig (mates on one edge)."""
    k, G, Lr = 31, 90000, 150
    rnd = random.Random(77)
    g_ = [rnd.choice("AGCT") for _ in range(G)]
    for a, b in ((2000, 5000), (8000, 11000)):
        g_[b:b + 300] = g_[a:a + 300]
    genome = "".join(g_)
    tiles = []
    for s in list(range(0, G - Lr + 1, 25)) + [G - Lr]:
        tiles += [genome[s:s + Lr], R.rev_comp(genome[s:s + Lr])]
    mates = []
    for i in range(3000):
        ins = rnd.randint(k + 185, k + 245)
        s = rnd.randrange(1000, 12500) if i % 3 else rnd.randrange(15000, G - ins)
        frag = genome[s:s + ins]
        if rnd.random() < 0.5:
            frag = R.rev_comp(frag)
        mates += [frag[:100], R.rev_comp(frag)[:100]]
    binb, pbin = dna.reads_to_bin(tiles + mates), dna.reads_to_bin(mates)
    nreads, npairs = len(tiles) + len(mates), len(mates) // 2
    og = oracle_graph(k, binb, nreads, 1)
    assert max(int(x) for x in og.edges()["len"]) > 65535
    nwalk = npairs if rng == RANGE else 300                 # (up to 65535 the oracle unrolls the repeats' cycles: 40 ms a walk)
    want = oracle_round(og, k, pbin, nwalk, rng, errors=False)
    m, g = device_graph(ctx, k, binb, nreads, 1)
    assert max(len(e[2]) for e in g.canonical()[1]) > 65535
    orientations, overflowed = device_round(ctx, g, k, want, [(pbin, nwalk)], rng)
    assert orientations == 2 * nwalk
    if rng == RANGE:
        assert overflowed < orientations
    g.close(); m.close()


# ---- d. walks that outgrow the LDS sets on their own -------------------------------------------------------------------------

BUSHY_ERR = 0.01


def bushy():
    k = 47
    reads = pairs(300, k, 100, err=BUSHY_ERR)
    return k, reads, dna.reads_to_bin(reads)


def test_natural_overflow_both_walkers_contribute_to_one_result(ctx):
    """An unfiltered graph (every k-mer kept) of reads with 1 % substitutions, k = 47, 100-base mates, range 180..250: tens of
    thousands of nodes, bubbles and tips within 250 bases of every mate.  With the DEFAULT set sizes (192 reached nodes, 384
    states, 96 pairs per wave) some orientations outgrow the LDS and go to the host walker, the others stay on the device:
    0 < overflowed < orientations, and the two walkers' counts add up to the oracle's exactly.
    Measured on an MI355X: 12 000 orientations handed over, 11 333 of them to the host walker, 667 walked by the kernel (33 028
    nodes; 25 734 support entries, 1 210 bad pairs).  The same reads at 0.5 % / 0.2 % / 2 % substitutions overflow 10 935 / 956 /
    9 947 of 12 000; with the count filter (min count 2) none does, at any k of case (a)."""
    k, reads, binb = bushy()
    npairs = len(reads) // 2
    want = oracle_round(oracle_graph(k, binb, len(reads), 1), k, binb, npairs, RANGE)
    m, g = device_graph(ctx, k, binb, len(reads), 1)
    orientations, overflowed = device_round(ctx, g, k, want, [(binb, npairs)], RANGE)
    print("natural overflow: orientations %d overflowed %d" % (orientations, overflowed))
    assert orientations == 2 * npairs
    assert 0 < overflowed < orientations
    g.close(); m.close()


def test_natural_overflow_fixture_on_the_host_walker_alone(ctx):
    """`pairs_host` = 1 on the same fixture: every orientation on the host walker by choice — the same five quantities, and no
    orientation counted as overflowed."""
    k, reads, binb = bushy()
    npairs = len(reads) // 2
    want = oracle_round(oracle_graph(k, binb, len(reads), 1), k, binb, npairs, RANGE)
    m, g = device_graph(ctx, k, binb, len(reads), 1)
    ctx.set_option("pairs_host", 1)
    try:
        orientations, overflowed = device_round(ctx, g, k, want, [(binb, npairs)], RANGE)
    finally:
        ctx.set_option("pairs_host", 0)
    assert (orientations, overflowed) == (2 * npairs, 0)
    g.close(); m.close()


# ---- e. mate shapes -------------------------------------------------------------------------------------------------------

def shape_stream(shape, k, seed):
    """-> (reads of the walked stream, npairs to walk).  Same seed, genome length, repeats
    and k as the graph's reads: make_pairs draws the same genome."""
    if shape == "255":
        return pairs(seed, k, 255), NPAIRS
    if shape == "exactly_k":
        return pairs(seed, k, k), NPAIRS
    reads = pairs(seed, k, 150)
    if shape == "first_record_short":                       # bin[0] < k: the whole stream takes the host cut, which skips that pair
        reads[0] = reads[0][:k - 1]
    elif shape == "last_pair_one_short":                     # same record size (38 payload bytes): the device cut sees the length byte
        reads[-1] = reads[-1][:-1]
    elif shape == "last_pair_one_byte_short":                # 101 -> 100 bases: one payload byte less, the stream is shorter than uniform
        reads = pairs(seed, k, 101)
        reads[-1] = reads[-1][:-1]
    elif shape == "alternating":                             # 150 / 100, swapping sides every pair
        for i in range(0, len(reads), 2):
            j = i + (i // 2) % 2
            reads[j] = reads[j][:100]
    elif shape == "zero_length_mate":
        for i in (1, 2 * 777, len(reads) - 1):
            reads[i] = ""
    elif shape == "npairs_below_stream":
        return reads, NPAIRS // 3
    return reads, NPAIRS


@pytest.mark.parametrize("shape", ["255", "exactly_k", "first_record_short", "last_pair_one_short", "last_pair_one_byte_short", "alternating",
                                   "npairs_below_stream", "zero_length_mate"])
def test_mate_shapes(ctx, shape):
    """k = 55, the graph of 150-base mates; the walked stream has the shape.  `l0 = bin[0]` decides the record size of the device
    cut and is compared as a byte: 255 is its limit, k its lower end (one k-mer per mate), a first record below k or any
    departure from uniform sends the stream to the host cut."""
    k, seed = 55, 555
    built = pairs(seed, k, 150)
    binb = dna.reads_to_bin(built)
    reads, npairs = shape_stream(shape, k, seed)
    lens = {len(r) for r in reads}
    assert {"255": lens == {255}, "exactly_k": lens == {k}, "first_record_short": lens == {k - 1, 150}, "last_pair_one_short": lens == {149, 150},
            "last_pair_one_byte_short": lens == {100, 101}, "alternating": lens == {100, 150}, "zero_length_mate": lens == {0, 150},
            "npairs_below_stream": lens == {150} and npairs < len(reads) // 2}[shape]
    wbin = dna.reads_to_bin(reads)
    want = oracle_round(oracle_graph(k, binb, len(built), 2), k, wbin, npairs, RANGE)
    m, g = device_graph(ctx, k, binb, len(built), 2)
    orientations, overflowed = device_round(ctx, g, k, want, [(wbin, npairs)], RANGE)
    skipped = {"first_record_short": 1, "last_pair_one_short": 0, "zero_length_mate": 3}.get(shape, 0)
    assert orientations == 2 * (npairs - skipped) and overflowed < orientations
    g.close(); m.close()


# ---- f. walks on an edited graph -----------------------------------------------------------------------------------------------

def test_two_rounds_on_an_edited_graph(ctx):
    """k = 63, every k-mer kept (0.2 % substitutions, no count filter: a fresh build of filtered reads has no bubble to remove and
    nothing to merge).  removeBubbles + simplifyGraph first: dead ids, id gaps and long edges, over which k_in_count / k_in_fill
    run.  Then getGraphMap -> walk -> split -> simplify, and the same again on the result, whose node copies share a sequence.
    The oracle does both rounds; every step is compared.  (device_round also checks that each round's stale position map raises
    on the graph the round leaves.)"""
    k = 63
    reads = pairs(663, k, 150, err=0.002)
    binb = dna.reads_to_bin(reads)
    npairs = len(reads) // 2
    fresh = oracle_graph(k, binb, len(reads), 1)
    og = oracle_graph(k, binb, len(reads), 1, edit=True)
    assert og.num_edges() < fresh.num_edges() and og.total_edge_len() < fresh.total_edge_len()      # the edit removed and merged
    want1 = oracle_round(og, k, binb, npairs, RANGE)
    want2 = oracle_round(og, k, binb, npairs, RANGE, split=False)
    assert want2["graph"] == want1["after"] and want2["split"] != (0, 0)
    m, g = device_graph(ctx, k, binb, len(reads), 1, edit=True)
    n_ids, e_ids = g.idBounds()
    assert g.counts()[1] < e_ids                                # the edit left dead edge ids behind
    o1, v1 = device_round(ctx, g, k, want1, [(binb, npairs)], RANGE)
    o2, v2 = device_round(ctx, g, k, want2, [(binb, npairs)], RANGE)
    assert v1 < o1 and v2 < o2
    g.close(); m.close()
