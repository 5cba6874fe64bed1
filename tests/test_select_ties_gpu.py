"""Every selection of the later engines -- a ranking, or the pick of a best or a worst -- on TIED fitness,
against the one contract of bbo_rank.hpp

    rank[i] = #{ j : f_j < f_i  or  (f_j == f_i and j < i) },   order[rank[i]] = i

and, for the picks, its two ends: the FIRST minimum and the FIRST maximum (bbo_wave.hpp: wave_argmin,
wave_argmax, block_arg<+-1>: "on a tie the lower index").  The reference is plain numpy on the fitness the
handle holds, read back and compared bit for bit with what was put in: a stable argsort for the orderings,
the first argmin / argmax for the picks.  Every comparison is exact.  The families and the reference are those
of test_rank_ties_gpu.py (tests/_tie_families.py).

Fitness goes in through set_state where the engine has such a key, else through a callback objective that
hands out the next value of the family (the rows arrive in index order: the *_callable_in_the_builtins_order_*
tests); through the callback the first value of every population is NaN, which must be stored as +inf (PIKAIA,
which maximises: as -inf, "a NaN ranks worst") and rank by its index among the other infinities.

SITES is the table of every selection site, written down from the kernels' launch conditions as they read,
not by calling the code.  An engine's header may state a rule that is not "ties by row index"; that rule, quoted,
is then the reference:

  ACD   bbo_acd_kernels.hpp, acd_ae: "The archive is ranked stably with respect to the persisting `order`
        ...: position k of the old order goes to the number of values below its own plus the equal ones in
        front of it."                                       ref = old[argsort(f[old], stable)]
  SSDE  bbo_ssde_kernels.hpp, ssde_sort: "the row of rank k goes to the place that pair_less (fitness, then the
        rank it had) gives it, so ties keep their order."   ref = old[argsort(f[old], stable)]
  CRS   crs_steps, update(): "the point into the worst's row, the row to its rank behind the values that are <=
        its own."      ref = the old order without its last entry, the row inserted at searchsorted(., "right")
  JAYA  jaya_partition: best and worst of a sub-population are the first in SLOT order (the shuffled order
        `occ`), not in row order; jaya_finish: "the incumbent (on a tie the lowest row)".
  PIKAIA  ascending fitness, ties by row: the best is order[np - 1], the LAST of the tied rows.
  CSO   cso_groups: "sort inside every group of pc consecutive slots by fitness (stable: ties keep the shuffled
        order ...)".  The shuffled order is read back through the read-only key `shuffled` (added for this: the
        order before the sort had no key; `home` is the order after it).
                                  ref, group by group = src[argsort(f[src], stable)], src = the group's slots

Dropped from the table, with the reason:
  APSO  pso_control_a's block_arg<1> / block_arg<-1> over the mean distances `ws`: only the two VALUES are
       used (evof), never the indices, so their tie rule has no observable outcome.  Its third block_arg, over
       f, is in the table.
  xNES np = 5: the population size is 4 + int(3 ln n), which skips 5 (n = 1 gives 4, n = 2 gives 6).
  PIKAIA, Mayfly: odd population sizes are refused by the constructors; the seams are taken at the even
       neighbours.  PIKAIA np = 2 (the engine's minimum) is below the families' minimum length 4 and runs a
       hand-made pair instead.
  SLPSO has no fitness sort (`perm` is a shuffle).  Its one pick, the swarm's best of slpso_init, is a
       sequential scan by one thread ("strict <, index order"): listed, without seams.
  SSDE `perm` is the coordinate permutation of a generation, not an order of the pool: nothing to hold it to.

That the cases bite was shown on four scratch builds of the library, one flipped comparison each (each still a
total order: valid permutations, valid indices); this file then failed in
  1  rank_by_counting, `j < cand` -> `j > cand`:  every case of lm_ranking, amalgam_ranking, crs_ranking,
     mayfly_rankings; and, through the ranking they also read, amalgam_best_ever and crs_new_point
  2  wave_argmin / wave_argmax, `os < s` -> `os > s`:  every case of nshs_best_and_worst, jaya_initial_incumbent,
     jaya_best_and_worst_of_a_sub_population, jaya_empty_lanes; 9 of 10 of mayfly_initial_best
  3  block_arg, `oi < idx` -> `oi > idx` (inside a wavefront):  every case of spiral_best, the three apso tests,
     amalgam_best_ever, mayfly_pgb, mayfly_merge, mayfly_rankings (the chain of fbest)
  4  block_arg, `sidx[w] < idx` -> `sidx[w] > idx` (across the four wavefronts):  the cases of the same tests
     that hold more than one wavefront of values
and passed everywhere else (xNES, PIKAIA, ACD, SSDE, CSO and SLPSO use none of the three primitives)."""
import numpy as np
import pytest

from _tie_families import FAMILIES, family, groups, bits, reference, check_family_claims

gpu = pytest.mark.gpu
INF = np.inf
COUNT_SEAMS = (4, 32, 33, 2047, 2048, 2049, 4096)        # rank_by_counting<8>: 32 candidates a workgroup, tile 2048
BLOCK_SEAMS = (5, 64, 65, 256, 257)                        # block_arg: lane, wavefront, the four wavefronts, the stride

# ---- the case tables ------------------------------------------------------------------------------------------
LM_CASES = [(L, P) for L in COUNT_SEAMS for P in (1, 2)]
AMALGAM_RANK_CASES = [(L, P) for L in COUNT_SEAMS for P in (1, 2)]
AMALGAM_BEST_CASES = [(L, P) for L in BLOCK_SEAMS for P in (1, 3)]
CRS_RANK_CASES = [(L, P) for L in COUNT_SEAMS for P in (1, 3)]
CRS_REPLACE_CASES = [(33, 1), (33, 3), (2049, 1)]
# Mayfly: np even.  (np, pmutnp, P): the swarms' ranking has np keys, the selection's np + np / 2 + nmut / 2
MAYFLY_GEN_CASES = [(4, 0.5, 1), (4, 0.5, 3), (32, 0.05, 1), (34, 0.5, 3), (2046, 0.05, 1), (2048, 0.05, 3),
                    (2050, 0.05, 1), (4096, 0.05, 3)]
MAYFLY_INIT_NP = (2, 32, 34, 66, 130)                      # 2 np values in one wavefront: 4, 64, 68, 132, 260
MAYFLY_PGB_NP = (4, 64, 66, 256, 258)                      # block_arg over the np females
MAYFLY_MERGE_NP = (4, 42, 44, 170, 172)                    # pmutnp = 0.5: np + nmut = 6, 64, 66, 256, 258


def mayfly_nmut(np_, pmutnp):
    nmut = int(pmutnp * np_)                               # bbo_mayfly.hip: c.nmut
    return min(nmut + 1, np_) if nmut % 2 else nmut


def xnes_np(n):
    return 4 + int(3. * np.log(1. * n))                    # xnes.cpp:63


XNES_N = {}                                                # np -> the smallest n that has it: every np from 4 to 22 but 5
for _n in range(512, 0, -1):
    XNES_N[xnes_np(_n)] = _n
PIKAIA_NP = (4, 62, 64, 66, 256, 258, 1000, 1024, 1026, 2048, 2050, 4094, 4096)
PIKAIA_CASES = [(L, P) for L in PIKAIA_NP for P in ((1, 3) if L <= 1026 else (1,))]
PIKAIA_ELITE_CASES = [(4, 1), (64, 3), (66, 1), (1026, 3)]
ACD_N = (2, 8, 9, 32, 33, 128)                             # 2 n keys, ACD_THREADS = 128 threads stride them
SSDE_NP = (4, 64, 65, 4096)
SSDE_GEN_CASES = [(4, 1), (4, 3), (64, 1), (64, 3), (65, 1), (65, 3), (4096, 3)]
JAYA_BEST_NP = (5, 64, 65, 256, 257, 1025)                 # jaya_finish: 256 threads stride the rows
# (np, k): k sub-populations of np / k slots (sizes 1, 2, 64, 65, 130; 131 = 65 + 66 or 66 + 65 by the engine's draw)
JAYA_SUB_CASES = [(5, 5), (8, 4), (128, 2), (130, 2), (260, 2), (131, 2)]
NSHS_HMS = (5, 64, 65, 130, 4096)                          # one wavefront strides the memory
SPIRAL_NP = (5, 64, 65, 256, 257, 1025)
APSO_NP = (30, 64, 65, 256, 257, 1024)
SLPSO_NP = (5, 257)
# CSO, (np, pcompete): 4, 256, 257 groups of 2 and 3, 256, 257 groups of 3
CSO_CASES = [(8, 2), (512, 2), (514, 2), (9, 3), (768, 3), (771, 3)]

# ---- the table of sites: engine, kernel, what it picks, the seams, the state keys that show it, the lengths run ----
SITES = [
    ("LmCMAES", "lm_rank",
     "order, rank, sorted values of lambda keys",
     "rank_by_counting<8>: 32 a workgroup, tile 2048",
     "fit_idx, fit_rank, fit_val", [c[0] for c in LM_CASES]),
    ("AMALGAM", "amalgam_rank",
     "order of np keys",
     "rank_by_counting<8>",
     "fit_idx", [c[0] for c in AMALGAM_RANK_CASES]),
    ("AMALGAM", "amalgam_adapt",
     "first minimum of np values, taken when it is not row 0 and beats fbest",
     "256 threads stride the rows, block_arg<1>",
     "xbest, fbest", [c[0] for c in AMALGAM_BEST_CASES]),
    ("CRS", "crs_rank",
     "order of np keys, fbest, fworst",
     "rank_by_counting<8>; the population in blockIdx.x",
     "order, f, fbest, fworst", [c[0] for c in CRS_RANK_CASES]),
    ("CRS", "crs_steps update()",
     "the new point's place behind the values <= its own",
     "binary search + shift by T threads",
     "order, f, rows", [c[0] for c in CRS_REPLACE_CASES]),
    ("Mayfly", "mayfly_rank which = 0",
     "order of the np males (z = 0) and the np females (z = 1)",
     "rank_by_counting<8>; population in blockIdx.x, swarm in blockIdx.z",
     "rank_m, rank_f", [c[0] for c in MAYFLY_GEN_CASES]),
    ("Mayfly", "mayfly_rank which = 1",
     "order of the cm = np + np / 2 + nmut / 2 records of each selection",
     "rank_by_counting<8>",
     "sel_m, sel_f", [c[0] + c[0] // 2 + mayfly_nmut(c[0], c[1]) // 2 for c in MAYFLY_GEN_CASES]),
    ("Mayfly", "mayfly_init_best",
     "first minimum over male 0, female 0, male 1, ...",
     "one wavefront strides 2 np values, wave_argmin",
     "fbest, xbest", [2 * m for m in MAYFLY_INIT_NP]),
    ("Mayfly", "mayfly_males (pgb)",
     "first minimum of the np females",
     "256 threads, block_arg<1>",
     "took, fbest, xbest", list(MAYFLY_PGB_NP)),
    ("Mayfly", "mayfly_merge",
     "first minimum of the np offspring then the nmut mutated flies",
     "256 threads, block_arg<1>",
     "took, fbest, xbest", [m + mayfly_nmut(m, 0.5) for m in MAYFLY_MERGE_NP]),
    ("xNES", "xnes_rank",
     "order of np keys",
     "one wavefront, a lane per candidate: every np from 4 to XNES_MAX_NP = 22",
     "fit_idx", sorted(XNES_N)),
    ("PIKAIA", "pikaia_newpop",
     "ascending order and rank of np keys, the best last",
     "bitonic_sort_lds, threads by rank_sort_m(np)",
     "order, rank", [c[0] for c in PIKAIA_CASES]),
    ("PIKAIA", "pikaia_newpop elite",
     "the row order[np - 1] of a tied top; the initial zeros",
     "as above",
     "elite, x, order", [c[0] for c in PIKAIA_ELITE_CASES]),
    ("ACD", "acd_ae",
     "order of the 2 n archive values, stable in the persisting order",
     "128 threads stride 2 n keys",
     "order", [2 * n for n in ACD_N]),
    ("SSDE", "ssde_init (ssde_sort)",
     "order of npinit and of 2 npinit rows from the identity",
     "256 threads stride the keys",
     "order, f", [m for L in SSDE_NP for m in (L, 2 * L)]),
    ("SSDE", "ssde_generation (ssde_sort)",
     "order of np rows, stable in the rank they had",
     "T threads stride the keys",
     "order, f", [c[0] for c in SSDE_GEN_CASES]),
    ("JAYA", "jaya_partition",
     "first minimum and first maximum of every sub-population in slot order",
     "a wavefront per sub-population strides its slots, wave_argmin / wave_argmax",
     "trial", [c[0] for c in JAYA_SUB_CASES]),
    ("JAYA", "jaya_finish",
     "first minimum of np values",
     "256 threads stride the rows, wave_argmin, four wavefronts",
     "bestx, fgbest", list(JAYA_BEST_NP) + [c[0] for c in JAYA_SUB_CASES]),
    ("NSHS", "nshs_select",
     "first minimum and first maximum of hms values",
     "one wavefront strides the memory",
     "ibest, iworst", list(NSHS_HMS)),
    ("SpiralSearch", "spiral_best",
     "first minimum of np values",
     "256 threads, block_arg<1>",
     "ibest, xbest, fbest", list(SPIRAL_NP)),
    ("APSO", "pso_gbest_init",
     "first minimum of np values",
     "256 threads, block_arg<1>",
     "xbest, fbest", list(APSO_NP)),
    ("APSO", "pso_control_a",
     "first minimum of f (the evolutionary factor reads ws there)",
     "third block_arg<1> of the kernel",
     "evof", list(APSO_NP)),
    ("APSO", "pso_control_b",
     "first maximum of f: the particle the elitist candidate replaces",
     "block_arg<-1>",
     "fb, xb", list(APSO_NP)),
    ("APSO", "pso_gbest, pso_finish",
     "first minimum of a chunk [i0, i1), then of the swarm; only a strictly better one is taken",
     "block_arg<1>; the chunk boundary splits the ties",
     "xbest, fbest", list(APSO_NP)),
    ("CSO", "cso_groups",
     "order inside every group of pcompete slots, stable in the shuffled order",
     "a thread per group, 256 a workgroup",
     "home, shuffled", [c[0] for c in CSO_CASES]),
    ("SLPSO", "slpso_init",
     "first minimum of np values",
     "one thread, index order: no seam",
     "abest, fabest", list(SLPSO_NP)),
]
ENGINES = ("SpiralSearch", "NSHS", "LmCMAES", "xNES", "AMALGAM", "SLPSO", "CRS", "SSDE", "ACD", "Mayfly", "PIKAIA", "JAYA",
           "APSO", "CSO")


def all_lengths():
    return sorted({L for s in SITES for L in s[5]})


def test_every_site_has_a_case_and_every_length_holds_its_ties():
    assert {s[0] for s in SITES} == set(ENGINES)
    for engine, kernel, picks, seams, keys, lengths in SITES:
        assert len(lengths) >= 1, (engine, kernel)
        assert all(L >= 4 for L in lengths), (engine, kernel)
    assert sorted(XNES_N) == [4] + list(range(6, 23))
    for L in all_lengths():
        check_family_claims(L)
    for P in (1, 2, 3):
        g = groups(P)
        assert all(len(h) == P for h in g) and {k for h in g for k in h} == set(range(7))


# ---- helpers -----------------------------------------------------------------------------------------------------
class Feed:
    """a callback objective that hands out the queued values in order; `rest` when the queue is empty"""

    def __init__(self, rest=0.):
        self.queue, self.rest, self.calls = [], rest, 0

    def __call__(self, x):
        self.calls += 1
        return self.queue.pop() if self.queue else self.rest

    def load(self, values):
        assert not self.queue
        self.queue = [float(v) for v in values][::-1]

    def empty(self):
        return not self.queue


def nan_first(v, stored=INF):
    """(what is handed out, what must be stored): the first value is NaN"""
    out, want = v.copy(), v.copy()
    out[0], want[0] = np.nan, stored
    return out, want


def box(n, half=5.):
    return -half * np.ones(n), half * np.ones(n)


def first_min(f):
    return int(np.argmin(f))                               # numpy: the first occurrence


def first_max(f):
    return int(np.argmax(f))


def same_bits(a, b, msg=""):
    np.testing.assert_array_equal(bits(a), bits(b), err_msg=msg)


def ints(a):
    return np.asarray(a).astype(np.int64)


# ---- LmCMAES ---------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("lam,P", LM_CASES, ids=["L%d-P%d" % c for c in LM_CASES])
def test_lm_ranking_is_the_stable_order(hip, lam, P):
    """sample, evaluate through the callback, rank: order, rank and the sorted values"""
    n = 2
    lo, hi = box(n)
    for fams in groups(P):
        feed = Feed()
        g = hip.LmCMAES(10 ** 9, 1e-12, lam, seed=2, populations=P)
        g.initialize(feed, lo, hi, np.zeros((P, n)))
        want, out = [], []
        for k in fams:
            o, w = nan_first(family(k, lam))
            out.extend(o)
            want.append(w)
        feed.load(out)
        g.phase(0)
        g.phase(1)
        assert feed.empty()
        g.phase(2)
        for p, k in enumerate(fams):
            msg = "%s, lambda = %d, population %d" % (FAMILIES[k], lam, p)
            f = g.get_state("f", p)
            same_bits(f, want[p], msg)
            order, rank = reference(f)
            np.testing.assert_array_equal(ints(g.get_state("fit_idx", p)), order, err_msg=msg)
            np.testing.assert_array_equal(ints(g.get_state("fit_rank", p)), rank, err_msg=msg)
            same_bits(g.get_state("fit_val", p), f[order], msg)


# ---- AMALGAM ---------------------------------------------------------------------------------------------------
def _amalgam(hip, np_, P, feed):
    n = 2
    lo, hi = box(n)
    g = hip.AMALGAM(10 ** 9, 0., 0., np=np_, noparam=False, print=False, seed=3, populations=P)
    g.initialize(feed, lo, hi, np.zeros((P, n)))
    return g


@gpu
@pytest.mark.parametrize("np_,P", AMALGAM_RANK_CASES, ids=["np%d-P%d" % c for c in AMALGAM_RANK_CASES])
def test_amalgam_ranking_is_the_stable_order(hip, np_, P):
    """the initial population through the callback, row by row, and the ranking that follows it"""
    for fams in groups(P):
        feed = Feed()
        want, out = [], []
        for k in fams:
            o, w = nan_first(family(k, np_))
            out.extend(o)
            want.append(w)
        feed.load(out)
        g = _amalgam(hip, np_, P, feed)
        assert feed.empty()
        for p, k in enumerate(fams):
            msg = "%s, np = %d, population %d" % (FAMILIES[k], np_, p)
            f = g.get_state("fit_val", p)
            same_bits(f, want[p], msg)
            np.testing.assert_array_equal(ints(g.get_state("fit_idx", p)), reference(f)[0], err_msg=msg)


@gpu
@pytest.mark.parametrize("np_,P", AMALGAM_BEST_CASES, ids=["np%d-P%d" % c for c in AMALGAM_BEST_CASES])
def test_amalgam_best_ever_is_the_first_minimum(hip, np_, P):
    """an initial population of +inf (fbest = +inf, xbest = row 0), then set_state("fit_val") and the adapt phase:
    the first minimum, when it is not row 0 and below fbest, gives xbest and fbest; the ranking follows"""
    n = 2
    for fams in groups(P):
        g = _amalgam(hip, np_, P, Feed(rest=INF))
        for p, k in enumerate(fams):
            g.set_state("fit_val", family(k, np_), p)
        g.phase(2)
        for p, k in enumerate(fams):
            msg = "%s, np = %d, population %d" % (FAMILIES[k], np_, p)
            f = g.get_state("fit_val", p)
            same_bits(f, family(k, np_), msg)
            x = g.get_state("arx", p).reshape(np_, n)
            assert np.unique(x, axis=0).shape[0] == np_, msg
            i = first_min(f)
            take = i > 0 and f[i] < INF
            same_bits(g.get_state("xbest", p), x[i if take else 0], msg)
            same_bits(g.get_state("fbest", p), [f[i] if take else INF], msg)
            np.testing.assert_array_equal(ints(g.get_state("fit_idx", p)), reference(f)[0], err_msg=msg)


# ---- CRS ---------------------------------------------------------------------------------------------------------
def _crs(hip, np_, P):
    n = 2
    lo, hi = box(n)
    g = hip.CRS(10 ** 9, np_, 0., seed=7, populations=P)
    g.initialize("sphere", lo, hi, np.zeros(P * n))
    return g


@gpu
@pytest.mark.parametrize("np_,P", CRS_RANK_CASES, ids=["np%d-P%d" % c for c in CRS_RANK_CASES])
def test_crs_ranking_is_the_stable_order(hip, np_, P):
    """set_state("f") and the ranking behind it: get_state("f") is in rank order"""
    for fams in groups(P):
        g = _crs(hip, np_, P)
        for p, k in enumerate(fams):
            g.set_state("f", family(k, np_), p)
        for p, k in enumerate(fams):
            msg = "%s, np = %d, population %d" % (FAMILIES[k], np_, p)
            f = family(k, np_)
            order, _ = reference(f)
            np.testing.assert_array_equal(ints(g.get_state("order", p)), order, err_msg=msg)
            same_bits(g.get_state("f", p), f[order], msg)
            same_bits(g.get_state("fbest", p), [f[order[0]]], msg)
            same_bits(g.get_state("fworst", p), [f[order[-1]]], msg)


def _crs_absorb(g, P, first, rest):
    """the iteration in progress, one value at a time: `first` for the first pending point of a population, `rest`
    for every later one (the mutated point, or a trial the recursion evaluates again)"""
    pending = g.phase(0)
    assert pending == P
    given = [0] * P
    while pending:
        for p in range(P):
            if int(g.get_state("pending", p)[0]):
                g.set_state("value", [first[p] if given[p] == 0 else rest[p]], p)
                given[p] += 1
        pending = g.phase(2)
        assert max(given) < 64
    return given


@gpu
@pytest.mark.parametrize("how", ["ulp_below_the_worst", "equal_to_the_worst"])
@pytest.mark.parametrize("np_,P", CRS_REPLACE_CASES, ids=["np%d-P%d" % c for c in CRS_REPLACE_CASES])
def test_crs_new_point_goes_behind_equal_values(hip, np_, P, how):
    """update() on tied pools.  One ulp below the worst value the trial is accepted at once.  Equal to the worst
    it is not (`ft >= fworst`): the mutated point follows and is given the value of the best group (one ulp
    below the worst where the whole pool ties), so it lands BEHIND every stored value equal to its own."""
    n = 2
    for fams in groups(P):
        g = _crs(hip, np_, P)
        for p, k in enumerate(fams):
            g.set_state("f", family(k, np_), p)
        old, f0, first, rest = [], [], [], []
        for p, k in enumerate(fams):
            f = family(k, np_)
            o = reference(f)[0]
            worst, best = f[o[-1]], f[o[0]]
            below = np.nextafter(worst, -INF)
            old.append(o)
            f0.append(f)
            if how == "ulp_below_the_worst":
                first.append(below)
                rest.append(below)
            else:
                first.append(worst)
                rest.append(best if best < worst else below)
        given = _crs_absorb(g, P, first, rest)
        for p, k in enumerate(fams):
            msg = "%s, np = %d, population %d, %s" % (FAMILIES[k], np_, p, how)
            assert int(g.get_state("it", p)[0]) == 1, msg
            assert given[p] >= (1 if how == "ulp_below_the_worst" else 2), msg
            v = rest[p]
            row, kept = old[p][-1], old[p][:-1]
            f = f0[p].copy()
            f[row] = v
            slot = int(np.searchsorted(f[kept], v, side="right"))
            want = np.concatenate([kept[:slot], [row], kept[slot:]])
            np.testing.assert_array_equal(ints(g.get_state("order", p)), want, err_msg=msg)
            same_bits(g.get_state("f", p), f[want], msg)
            point = g.get_state("rows", p).reshape(np_, n)[row]
            cands = [g.get_state("cand", p), g.get_state("cand2", p)]
            assert any(np.array_equal(bits(point), bits(c)) for c in cands), msg


# ---- Mayfly ------------------------------------------------------------------------------------------------------
def _mayfly(hip, np_, P, feed, **kw):
    n = 2
    lo, hi = box(n)
    g = hip.Mayfly(np_, 10 ** 9, seed=9, populations=P, **kw)
    g.initialize(feed, lo, hi, np.zeros(P * n))
    return g


def _mayfly_generation(g, feed, P, np_, nmut, fem, mal, off, mut):
    """one generation with the values of the callback in the order the engine asks for them: the females of
    population 0, 1, ..; male j of population 0, 1, .. for j = 0, 1, ..; the offspring; the mutated flies"""
    out = []
    for p in range(P):
        out.extend(fem[p])
    for j in range(np_):
        for p in range(P):
            out.append(mal[p][j])
    for p in range(P):
        out.extend(off[p])
    for p in range(P):
        out.extend(mut[p])
    feed.load(out)
    g.iterate()
    assert feed.empty()


@gpu
@pytest.mark.parametrize("np_,pmutnp,P", MAYFLY_GEN_CASES, ids=["np%d-pm%g-P%d" % c for c in MAYFLY_GEN_CASES])
def test_mayfly_rankings_are_the_stable_order(hip, np_, pmutnp, P):
    """a generation on swarms that start at +inf: the females, the males, the offspring and the mutated flies of a
    population take four different families (a swapped blockIdx.z shows).  The two rankings of the swarms, the two
    of the selections' records (np flies in rank order, half the shuffled offspring, half the shuffled mutated
    flies) and the chain of fbest: the first male that is strictly better, then the first minimum of offspring and
    mutated flies when it is strictly better again."""
    nmut, h = mayfly_nmut(np_, pmutnp), np_ // 2
    hm = nmut // 2
    for fams in groups(P):
        feed = Feed(rest=INF)
        g = _mayfly(hip, np_, P, feed, pmutnp=pmutnp)
        assert int(g.get_state("nmut")[0]) == nmut
        fem, mal, off, mut = [], [], [], []
        for k in fams:
            o, w = nan_first(family(k, np_))
            fem.append((o, w))
            mal.append(family((k + 1) % 7, np_))
            off.append(family((k + 2) % 7, np_))
            mut.append(family((k + 3) % 7, nmut) if nmut >= 4 else np.full(nmut, 2.5))
        _mayfly_generation(g, feed, P, np_, nmut, [v[0] for v in fem], mal, off, mut)
        for p, k in enumerate(fams):
            msg = "%s, np = %d, population %d" % (FAMILIES[k], np_, p)
            Ff, Mf = g.get_state("moved_females_f", p), g.get_state("moved_males_f", p)
            Of, Uf = g.get_state("off_f", p), g.get_state("mut_f", p)
            same_bits(Ff, fem[p][1], msg)
            same_bits(Mf, mal[p], msg)
            same_bits(Of, off[p], msg)
            same_bits(Uf, mut[p], msg)
            om, of_ = reference(Mf)[0], reference(Ff)[0]
            np.testing.assert_array_equal(ints(g.get_state("rank_m", p)), om, err_msg=msg)
            np.testing.assert_array_equal(ints(g.get_state("rank_f", p)), of_, err_msg=msg)
            po, pu = ints(g.get_state("perm_o", p)), ints(g.get_state("perm_u", p))
            keys_m = np.concatenate([Mf[om], Of[po[:h]], Uf[pu[:hm]]])
            keys_f = np.concatenate([Ff[of_], Of[po[h:2 * h]], Uf[pu[hm:2 * hm]]])
            np.testing.assert_array_equal(ints(g.get_state("sel_m", p)), reference(keys_m)[0], err_msg=msg)
            np.testing.assert_array_equal(ints(g.get_state("sel_f", p)), reference(keys_f)[0], err_msg=msg)
            fb, took = INF, -1
            i = first_min(Mf)
            if Mf[i] < fb:
                fb, took = Mf[i], np_ + i
            both = np.concatenate([Of, Uf])
            i = first_min(both)
            if both[i] < fb:
                fb, took = both[i], 2 * np_ + i
            assert int(g.get_state("took", p)[0]) == took, msg
            same_bits(g.get_state("fbest", p), [fb], msg)


@gpu
@pytest.mark.parametrize("pgb", [True, False])
@pytest.mark.parametrize("np_", MAYFLY_INIT_NP)
def test_mayfly_initial_best_is_the_first_minimum(hip, np_, pgb):
    """mayfly_init_best: the callback's order male 0, female 0, male 1, .. is the order of the scan; without pgb
    the females do not take part.  The point is the one the fly drew (kept as its velocity)."""
    n, L = 2, 2 * np_
    for P in (1, 3):
        for fams in groups(P):
            feed = Feed()
            out, want = [], []
            for k in fams:
                o, w = nan_first(family(k, L))
                out.extend(o)
                want.append(w)
            feed.load(out)
            g = _mayfly(hip, np_, P, feed, pgb=pgb)
            assert feed.empty()
            for p, k in enumerate(fams):
                msg = "%s, np = %d, population %d" % (FAMILIES[k], np_, p)
                Mf, Ff = g.get_state("males_f", p), g.get_state("females_f", p)
                same_bits(Mf, want[p][0::2], msg)
                same_bits(Ff, want[p][1::2], msg)
                scan = want[p].copy()
                if not pgb:
                    scan[1::2] = INF
                at = first_min(scan)                 # (every value +inf: male 0, which is the first minimum as well)
                drawn = g.get_state("females_v" if at & 1 else "males_v", p).reshape(np_, n)
                same_bits(g.get_state("fbest", p), [scan[at]], msg)
                same_bits(g.get_state("xbest", p), drawn[at >> 1], msg)
                same_bits(g.get_state("males_bf", p), Mf, msg)


@gpu
@pytest.mark.parametrize("np_", MAYFLY_PGB_NP)
def test_mayfly_pgb_takes_the_first_best_female(hip, np_):
    """pgb: before the male loop the first minimum of the moved females takes fbest.  Everything else is +inf."""
    n = 2
    for P in (1, 3):
        for fams in groups(P):
            feed = Feed(rest=INF)
            g = _mayfly(hip, np_, P, feed, pgb=True)
            nmut = int(g.get_state("nmut")[0])
            fem = [nan_first(family(k, np_)) for k in fams]
            inf = [np.full(np_, INF)] * P
            _mayfly_generation(g, feed, P, np_, nmut, [v[0] for v in fem], inf, inf, [np.full(nmut, INF)] * P)
            for p, k in enumerate(fams):
                msg = "%s, np = %d, population %d" % (FAMILIES[k], np_, p)
                Ff = g.get_state("moved_females_f", p)
                same_bits(Ff, fem[p][1], msg)
                i = first_min(Ff)
                took = i if Ff[i] < INF else -1
                assert int(g.get_state("took", p)[0]) == took, msg
                same_bits(g.get_state("fbest", p), [Ff[i]], msg)
                if took >= 0:
                    same_bits(g.get_state("xbest", p), g.get_state("moved_females_x", p).reshape(np_, n)[i], msg)


@gpu
@pytest.mark.parametrize("np_", MAYFLY_MERGE_NP)
def test_mayfly_merge_takes_the_first_best_child(hip, np_):
    """mayfly_merge: the family runs over the offspring and on into the mutated flies; the swarms stay at +inf"""
    n = 2
    nmut = mayfly_nmut(np_, 0.5)
    for P in (1, 3):
        for fams in groups(P):
            feed = Feed(rest=INF)
            g = _mayfly(hip, np_, P, feed, pmutnp=0.5)
            assert int(g.get_state("nmut")[0]) == nmut
            both = [family(k, np_ + nmut) for k in fams]
            inf = [np.full(np_, INF)] * P
            _mayfly_generation(g, feed, P, np_, nmut, inf, inf, [v[:np_] for v in both], [v[np_:] for v in both])
            for p, k in enumerate(fams):
                msg = "%s, np = %d, population %d" % (FAMILIES[k], np_, p)
                held = np.concatenate([g.get_state("off_f", p), g.get_state("mut_f", p)])
                same_bits(held, both[p], msg)
                i = first_min(held)
                took = 2 * np_ + i if held[i] < INF else -1
                assert int(g.get_state("took", p)[0]) == took, msg
                same_bits(g.get_state("fbest", p), [held[i]], msg)
                if took >= 0:
                    if i < np_:
                        x = g.get_state("off_x", p).reshape(np_, n)[i]
                    else:
                        x = g.get_state("mut_x", p).reshape(nmut, n)[i - np_]
                    same_bits(g.get_state("xbest", p), x, msg)


# ---- xNES --------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("P", [1, 3])
@pytest.mark.parametrize("np_", sorted(XNES_N))
def test_xnes_ranking_is_the_stable_order(hip, np_, P):
    n = XNES_N[np_]
    lo, hi = box(n)
    for fams in groups(P):
        feed = Feed()
        g = hip.xNES(10 ** 9, 0., seed=4, populations=P)
        g.initialize(feed, lo, hi, np.zeros(P * n))
        assert int(g.get_state("np")[0]) == np_
        out, want = [], []
        for k in fams:
            o, w = nan_first(family(k, np_))
            out.extend(o)
            want.append(w)
        feed.load(out)
        g.phase(0)
        assert feed.empty()
        g.phase(1)
        for p, k in enumerate(fams):
            msg = "%s, np = %d, population %d" % (FAMILIES[k], np_, p)
            f = g.get_state("fit_val", p)
            same_bits(f, want[p], msg)
            np.testing.assert_array_equal(ints(g.get_state("fit_idx", p)), reference(f)[0], err_msg=msg)


# ---- PIKAIA ------------------------------------------------------------------------------------------------------
def _pikaia(hip, np_, P, feed, **kw):
    n = 2
    g = hip.PIKAIA(np_, 1000, 9, pcross=1., imut=1, pmut=0.25, raw=True, seed=6, populations=P, **kw)
    g.initialize(feed, np.zeros(n), np.ones(n), np.zeros(P * n))
    return g


@gpu
@pytest.mark.parametrize("np_,P", PIKAIA_CASES, ids=["np%d-P%d" % c for c in PIKAIA_CASES])
def test_pikaia_ranking_is_the_stable_order(hip, np_, P):
    """raw: the fitness is the callback's value, a NaN is stored as -inf.  Ascending, ties by row."""
    for fams in groups(P):
        feed = Feed()
        g = _pikaia(hip, np_, P, feed)
        out, want = [], []
        for k in fams:
            o, w = nan_first(family(k, np_), stored=-INF)
            out.extend(o)
            want.append(w)
        feed.load(out)
        g.iterate()
        assert feed.empty()
        for p, k in enumerate(fams):
            msg = "%s, np = %d, population %d" % (FAMILIES[k], np_, p)
            f = g.get_state("fitns", p)
            same_bits(f, want[p], msg)
            order, rank = reference(f)
            np.testing.assert_array_equal(ints(g.get_state("order", p)), order, err_msg=msg)
            np.testing.assert_array_equal(ints(g.get_state("rank", p)), rank, err_msg=msg)


@gpu
def test_pikaia_pair_of_equal_values_keeps_its_rows(hip):
    """np = 2, the engine's minimum, below the families' shortest length"""
    for v in (1., INF, -INF, np.nan):
        feed = Feed()
        g = _pikaia(hip, 2, 1, feed)
        feed.load([v, v])
        g.iterate()
        assert [int(i) for i in g.get_state("order")] == [0, 1] and [int(i) for i in g.get_state("rank")] == [0, 1]


@gpu
@pytest.mark.parametrize("np_,P", PIKAIA_ELITE_CASES, ids=["np%d-P%d" % c for c in PIKAIA_ELITE_CASES])
def test_pikaia_elite_is_the_last_row_of_a_tied_top(hip, np_, P):
    """the initial state (every fitness 0 but the last row's) for a last value below and above 0; then, with
    ielite = 1, a generation that leaves a family behind and one whose new row 0 loses the elite test: the row
    that comes back is order[np - 1], the LAST of the tied best rows"""
    n = 2
    for last in (-1., 1.):
        g = _pikaia(hip, np_, P, Feed(rest=last))
        for p in range(P):
            f = g.get_state("fitns", p)
            same_bits(f, [0.] * (np_ - 1) + [last])
            order, rank = reference(f)
            np.testing.assert_array_equal(ints(g.get_state("order", p)), order)
            np.testing.assert_array_equal(ints(g.get_state("rank", p)), rank)
            assert order[0] == (np_ - 1 if last < 0. else 0)
    for fams in groups(P):
        feed = Feed(rest=1.)
        g = _pikaia(hip, np_, P, feed, ielite=1)
        # new row 0 of every population first (+inf: it wins the elite test), then the rows of every population
        out, want = [INF] * P, []
        for k in fams:
            o, w = nan_first(family(k, np_), stored=-INF)
            out.extend(o)
            want.append(w)
        feed.load(out)
        g.iterate()
        assert feed.empty()
        held = []
        for p, k in enumerate(fams):
            msg = "%s, np = %d, population %d" % (FAMILIES[k], np_, p)
            f = g.get_state("fitns", p)
            same_bits(f, want[p], msg)
            order = reference(f)[0]
            np.testing.assert_array_equal(ints(g.get_state("order", p)), order, err_msg=msg)
            assert int(g.get_state("elite", p)[0]) == 0, msg
            held.append((f, order, g.get_state("x", p).reshape(np_, n), g.get_state("ph", p).reshape(np_, n)))
        # new row 0 loses (-inf is below every top value here), the rows then take any values
        feed.load([-INF] * P + [1.] * (P * np_))
        g.iterate()
        assert feed.empty()
        for p, k in enumerate(fams):
            msg = "%s, np = %d, population %d" % (FAMILIES[k], np_, p)
            f, order, x, ph = held[p]
            top = order[-1]
            tied = np.flatnonzero(f == f[top])
            assert top == tied[-1], msg
            if tied.size > 1:        # a wrong pick among the tied rows shows: they are not all the same point
                assert any(not np.array_equal(x[i], x[top]) for i in tied), msg
            assert int(g.get_state("elite", p)[0]) == 1, msg
            same_bits(g.get_state("x", p).reshape(np_, n)[0], x[top], msg)
            same_bits(g.get_state("ph", p).reshape(np_, n)[0], ph[top], msg)


# ---- ACD ---------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("P", [1, 3])
@pytest.mark.parametrize("n", ACD_N)
def test_acd_archive_ranking_is_stable_in_the_persisting_order(hip, n, P):
    """the last coordinate step of a sweep that improved: its two values complete the family in the archive, then
    acd_ae ranks it.  Twice: from the reversed order that set_state("order") puts there, and from the order the
    first update leaves behind."""
    L = 2 * n
    lo, hi = box(n)
    rng = np.random.default_rng(n)
    for fams in groups(P):
        g = hip.ACD(10 ** 9, 0., 0., seed=8, populations=P)
        g.initialize("sphere", lo, hi, np.zeros(P * n))
        old = []
        for p in range(P):
            g.set_state("x", rng.uniform(-4., 4., (L, n)), p)
            g.set_state("order", np.arange(L)[::-1], p)
            old.append(np.arange(L)[::-1])
        for turn in range(2):
            want = [family((k + turn) % 7, L) for k in fams]
            for p in range(P):
                hold = want[p].copy()
                hold[L - 2:] = 0.5                    # (the step's two values overwrite these)
                g.set_state("f", hold, p)
                g.set_state("ix", [n - 1.], p)
                g.set_state("improved", [1.], p)
            assert g.phase(0) == P
            for p in range(P):
                g.set_state("value", want[p][L - 2:], p)
            g.phase(2)
            for p, k in enumerate(fams):
                msg = "%s, n = %d, population %d, update %d" % (FAMILIES[(k + turn) % 7], n, p, turn)
                assert int(g.get_state("due", p)[0]) == 0 and int(g.get_state("itae", p)[0]) == turn + 1, msg
                f = g.get_state("f", p)
                same_bits(f, want[p], msg)
                ref = old[p][np.argsort(f[old[p]], kind="stable")]
                np.testing.assert_array_equal(ints(g.get_state("order", p)), ref, err_msg=msg)
                old[p] = ref


# ---- SSDE --------------------------------------------------------------------------------------------------------
def _ssde(hip, npinit, P, feed, **kw):
    n = 2
    lo, hi = box(n)
    g = hip.SSDE(10 ** 9, npinit, 0., seed=5, populations=P, **kw)
    g.initialize(feed, lo, hi, np.zeros(P * n))
    return g


@gpu
@pytest.mark.parametrize("usede", [False, True])
@pytest.mark.parametrize("P", [1, 3])
@pytest.mark.parametrize("npinit", SSDE_NP)
def test_ssde_initial_ranking_is_the_stable_order(hip, npinit, P, usede):
    """the initial pool through the callback: npinit rows, with usede their opposites behind them; the best npinit
    stay.  get_state("f") is in rank order."""
    rows = 2 * npinit if usede else npinit
    for fams in groups(P):
        feed = Feed()
        out, want = [], []
        for k in fams:
            o, w = nan_first(family(k, rows))
            out.extend(o)
            want.append(w)
        feed.load(out)
        g = _ssde(hip, npinit, P, feed, usede=usede)
        assert feed.empty()
        for p, k in enumerate(fams):
            msg = "%s, %d rows, population %d" % (FAMILIES[k], rows, p)
            assert int(g.get_state("np", p)[0]) == npinit, msg
            order = reference(want[p])[0][:npinit]
            np.testing.assert_array_equal(ints(g.get_state("order", p)), order, err_msg=msg)
            same_bits(g.get_state("f", p), want[p][order], msg)


@gpu
@pytest.mark.parametrize("npinit,P", SSDE_GEN_CASES, ids=["np%d-P%d" % c for c in SSDE_GEN_CASES])
def test_ssde_generation_ranking_is_stable_in_the_rank_it_had(hip, npinit, P):
    """a generation on a pool whose order is not the identity.  Member i (the row of rank i) takes the i-th value
    of the next family where that is `<=` its own (select(): `if (!(f <= fi)) return false`), then the pool is
    sorted by (fitness, the rank it had)."""
    for fams in groups(P):
        feed = Feed()
        out, pool = [], []
        for k in fams:
            o, w = nan_first(family(k, npinit))
            out.extend(o)
            pool.append(w)
        feed.load(out)
        g = _ssde(hip, npinit, P, feed)
        old = [reference(f)[0] for f in pool]
        trial = [nan_first(family((k + 1) % 7, npinit)) for k in fams]
        out = []
        for i in range(npinit):                      # member i of population 0, 1, ..
            for p in range(P):
                out.append(trial[p][0][i])
        feed.load(out)
        g.iterate()
        assert feed.empty()
        for p, k in enumerate(fams):
            msg = "%s over %s, npinit = %d, population %d" % (FAMILIES[(k + 1) % 7], FAMILIES[k], npinit, p)
            f, t = pool[p].copy(), trial[p][1]
            rows = old[p]
            take = t <= f[rows]
            f[rows[take]] = t[take]
            ref = rows[np.argsort(f[rows], kind="stable")]
            now = int(g.get_state("np", p)[0])
            assert npinit - 1 <= now <= npinit, msg
            np.testing.assert_array_equal(ints(g.get_state("order", p)), ref[:now], err_msg=msg)
            same_bits(g.get_state("f", p), f[ref[:now]], msg)


# ---- JAYA --------------------------------------------------------------------------------------------------------
def _jaya(hip, np_, npmin, k0, P, feed):
    n = 2
    g = hip.JAYA(10 ** 9, 0., np_, npmin, adapt=False, k0=k0, mutation=hip.JAYA.original, seed=12, populations=P)
    g.initialize(feed, -1e6 * np.ones(n), 1e6 * np.ones(n), np.zeros(P * n))
    return g


@gpu
@pytest.mark.parametrize("P", [1, 3])
@pytest.mark.parametrize("np_", JAYA_BEST_NP)
def test_jaya_initial_incumbent_is_the_first_minimum(hip, np_, P):
    n = 2
    for fams in groups(P):
        feed = Feed()
        out, want = [], []
        for k in fams:
            o, w = nan_first(family(k, np_))
            out.extend(o)
            want.append(w)
        feed.load(out)
        g = _jaya(hip, np_, np_, 1, P, feed)
        assert feed.empty()
        for p, k in enumerate(fams):
            msg = "%s, np = %d, population %d" % (FAMILIES[k], np_, p)
            f = g.get_state("f", p)
            same_bits(f, want[p], msg)
            i = first_min(f)
            same_bits(g.get_state("fgbest", p), [f[i]], msg)
            if f[i] < INF:
                same_bits(g.get_state("bestx", p), g.get_state("X", p).reshape(np_, n)[i], msg)


def _jaya_generation_check(g, P, np_, k0, X, fs, msgs):
    """after one generation whose trials were all +inf (nothing is replaced): every trial row is the one its
    sub-population's FIRST best and FIRST worst slot give, in the kernel's operation order
        t = (x + r1 (best - |x|)) - r2 (worst - |x|)
    with r1, r2 the recorded draws; then the incumbent is the first minimum by row"""
    n = 2
    for p in range(P):
        msg = msgs[p]
        f = g.get_state("f", p)
        same_bits(f, fs[p], msg)
        same_bits(g.get_state("X", p), X.ravel(), msg)
        occ, lens = ints(g.get_state("occ", p)), ints(g.get_state("len", p))[:k0]
        assert sorted(occ) == list(range(np_)) and lens.sum() == np_ and lens.min() >= np_ // k0, msg
        trial = g.get_state("trial", p).reshape(np_, n)
        r = g.get_state("draws", p)[:-1].reshape(np_, n, 2)
        s0 = 0
        for q in range(k0):
            rows = occ[s0:s0 + lens[q]]
            s0 += lens[q]
            b, w = X[rows[first_min(f[rows])]], X[rows[first_max(f[rows])]]
            x, ax = X[rows], np.abs(X[rows])
            want = (x + r[rows, :, 0] * (b - ax)) - r[rows, :, 1] * (w - ax)
            assert np.abs(want).max() < 1e6, msg           # (inside the box: nothing is clamped)
            same_bits(trial[rows], want, msg + ", sub-population %d" % q)
        i = first_min(f)
        same_bits(g.get_state("fgbest", p), [f[i]], msg)
        if f[i] < INF:
            same_bits(g.get_state("bestx", p), X[i], msg)


@gpu
@pytest.mark.parametrize("P", [1, 3])
@pytest.mark.parametrize("np_,k0", JAYA_SUB_CASES, ids=["np%d-k%d" % c for c in JAYA_SUB_CASES])
def test_jaya_best_and_worst_of_a_sub_population_are_the_first_in_slot_order(hip, np_, k0, P):
    X = np.stack([np.arange(1., np_ + 1.), -0.5 * np.arange(1., np_ + 1.)], axis=1)      # row i is told by its tag
    for fams in groups(P):
        g = _jaya(hip, np_, np_ // k0, k0, P, Feed(rest=INF))
        g.set_state("record_draws", [1.])
        for p, k in enumerate(fams):
            g.set_state("X", X, p)
            g.set_state("f", family(k, np_), p)
        g.iterate()
        msgs = ["%s, np = %d, k = %d, population %d" % (FAMILIES[k], np_, k0, p) for p, k in enumerate(fams)]
        _jaya_generation_check(g, P, np_, k0, X, [family(k, np_) for k in fams], msgs)


@gpu
@pytest.mark.parametrize("np_,k0", [(8, 4), (130, 2), (260, 2)])
def test_jaya_empty_lanes_never_win(hip, np_, k0):
    """every value +inf in one population, every value -inf in the next: the lanes' initial (+-inf, INT_MAX) ties
    the values and must lose to every real slot"""
    X = np.stack([np.arange(1., np_ + 1.), -0.5 * np.arange(1., np_ + 1.)], axis=1)
    g = _jaya(hip, np_, np_ // k0, k0, 2, Feed(rest=INF))
    g.set_state("record_draws", [1.])
    fs = [np.full(np_, INF), np.full(np_, -INF)]
    for p in range(2):
        g.set_state("X", X, p)
        g.set_state("f", fs[p], p)
    g.iterate()
    _jaya_generation_check(g, 2, np_, k0, X, fs, ["all +inf", "all -inf"])


# ---- NSHS --------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("P", [1, 3])
@pytest.mark.parametrize("hms", NSHS_HMS)
def test_nshs_best_and_worst_are_the_first_of_their_ties(hip, hms, P):
    n = 2
    lo, hi = box(n)
    for fams in groups(P):
        g = hip.NSHS(10 ** 9, hms, seed=10, populations=P)
        g.initialize("sphere", lo, hi, np.zeros(P * n))
        for p, k in enumerate(fams):
            g.set_state("f", family(k, hms), p)
        for p, k in enumerate(fams):
            msg = "%s, hms = %d, population %d" % (FAMILIES[k], hms, p)
            f = g.get_state("f", p)
            same_bits(f, family(k, hms), msg)
            assert int(g.get_state("ibest", p)[0]) == first_min(f), msg
            assert int(g.get_state("iworst", p)[0]) == first_max(f), msg
            same_bits(g.get_state("fbest", p), [f[first_min(f)]], msg)       # (the value AT the pick: -0.0 is not +0.0)
            same_bits(g.get_state("fworst", p), [f[first_max(f)]], msg)
            same_bits(g.get_state("xbest", p), g.get_state("x", p).reshape(hms, n)[first_min(f)], msg)


# ---- SpiralSearch ------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("P", [1, 3])
@pytest.mark.parametrize("np_", SPIRAL_NP)
def test_spiral_best_is_the_first_minimum(hip, np_, P):
    """spiral_best behind the initial evaluation, and again behind the evaluate phase of a generation"""
    n = 2
    lo, hi = box(n)
    for fams in groups(P):
        feed = Feed()
        want = []
        for turn in range(2):
            out, want = [], []
            for k in fams:
                o, w = nan_first(family((k + turn) % 7, np_))
                out.extend(o)
                want.append(w)
            feed.load(out)
            if turn == 0:
                g = hip.SpiralSearch(10 ** 9, 0., np=np_, seed=11, populations=P)
                g.initialize(feed, lo, hi, np.zeros(P * n))
            else:
                g.phase(2)
                g.phase(3)
            assert feed.empty()
            for p, k in enumerate(fams):
                msg = "%s, np = %d, population %d, turn %d" % (FAMILIES[(k + turn) % 7], np_, p, turn)
                f = g.get_state("f", p)
                same_bits(f, want[p], msg)
                i = first_min(f)
                assert int(g.get_state("ibest", p)[0]) == i, msg
                same_bits(g.get_state("fbest", p), [f[i]], msg)
                same_bits(g.get_state("xbest", p), g.get_state("x", p).reshape(np_, n)[i], msg)


# ---- APSO --------------------------------------------------------------------------------------------------------
def _apso(hip, np_, P, feed):
    n = 2
    lo, hi = box(n)
    g = hip.APSO(10 ** 9, 0., np_, seed=13, populations=P)
    g.initialize(feed, lo, hi, np.zeros(P * n))
    return g


@gpu
@pytest.mark.parametrize("P", [1, 3])
@pytest.mark.parametrize("np_", APSO_NP)
def test_apso_initial_best_is_the_first_minimum(hip, np_, P):
    n = 2
    for fams in groups(P):
        feed = Feed()
        out, want = [], []
        for k in fams:
            o, w = nan_first(family(k, np_))
            out.extend(o)
            want.append(w)
        feed.load(out)
        g = _apso(hip, np_, P, feed)
        assert feed.empty()
        for p, k in enumerate(fams):
            msg = "%s, np = %d, population %d" % (FAMILIES[k], np_, p)
            f = g.get_state("f", p)
            same_bits(f, want[p], msg)
            x = g.get_state("x", p).reshape(np_, n)
            assert np.unique(x, axis=0).shape[0] == np_, msg
            i = first_min(f)
            same_bits(g.get_state("fbest", p), [f[i]], msg)
            same_bits(g.get_state("xbest", p), x[i], msg)


def _ring(np_, centre):
    """particle `centre` at the origin, the others evenly on the unit circle: its mean distance is the least"""
    a = 2. * np.pi * np.arange(np_) / np_
    x = np.stack([np.cos(a), np.sin(a)], axis=1)
    x[centre] = 0.
    return x


@gpu
@pytest.mark.parametrize("P", [1, 3])
@pytest.mark.parametrize("np_", APSO_NP)
def test_apso_control_picks_the_first_best_and_the_first_worst(hip, np_, P):
    """pso_control_a reads the mean distance `ws` of the FIRST minimum of f: with that particle in the middle of a
    ring evof is 0, the state becomes 3 (convergence) and the elitist candidate is evaluated.  Its value 0 does
    not beat fbest = -inf, so pso_control_b puts it in place of the FIRST maximum of f, whose own best (+inf)
    it beats; the moved swarm then evaluates to +inf and no other fb changes."""
    for fams in groups(P):
        feed = Feed(rest=INF)
        g = _apso(hip, np_, P, feed)
        held = []
        for p, k in enumerate(fams):
            f = family(k, np_)
            g.set_state("x", _ring(np_, first_min(f)), p)
            g.set_state("xb", _ring(np_, first_min(f)), p)
            g.set_state("f", f, p)
            g.set_state("fb", np.full(np_, INF), p)
            g.set_state("fbest", [-INF], p)
            held.append(f)
        feed.load([0.] * P)                           # the elitist candidates, population by population
        g.iterate()
        assert feed.empty() and feed.calls == 2 * P * np_ + P
        for p, k in enumerate(fams):
            msg = "%s, np = %d, population %d" % (FAMILIES[k], np_, p)
            f, ws = held[p], g.get_state("ws", p)
            lo_, hi_ = ws.min(), ws.max()
            assert hi_ > lo_, msg
            same_bits(g.get_state("evof", p), [(ws[first_min(f)] - lo_) / (hi_ - lo_)], msg)
            assert g.get_state("evof", p)[0] == 0. and int(g.get_state("state", p)[0]) == 3, msg
            fb = np.full(np_, INF)
            fb[first_max(f)] = 0.
            same_bits(g.get_state("fb", p), fb, msg)


@gpu
@pytest.mark.parametrize("P", [1, 3])
@pytest.mark.parametrize("np_", APSO_NP)
def test_apso_chunked_best_is_the_first_strict_improvement(hip, np_, P):
    """a generation in chunks of np // 2 + 1 particles (the boundary splits every run of ties): pso_gbest after the
    first chunk, pso_finish over the swarm.  The particle that is best before the move stands apart from a
    cluster, so evof is 1, the state 4 and no elitist candidate is evaluated."""
    n, chunk = 2, np_ // 2 + 1
    rng = np.random.default_rng(np_)
    x0 = np.concatenate([[[4.5, 4.5]], rng.uniform(-4.5, -3.5, (np_ - 1, n))])
    for fams in groups(P):
        feed = Feed(rest=INF)
        g = _apso(hip, np_, P, feed)
        g.set_state("chunk", [float(chunk)])
        want = [nan_first(family(k, np_)) for k in fams]
        for p in range(P):
            g.set_state("x", x0, p)
            g.set_state("xb", x0, p)
            g.set_state("f", np.arange(1., np_ + 1.), p)
            g.set_state("fb", np.full(np_, INF), p)
            g.set_state("fbest", [INF], p)
        out = []
        for i0 in range(0, np_, chunk):               # every chunk: population 0, 1, ..
            for p in range(P):
                out.extend(want[p][0][i0:i0 + chunk])
        feed.load(out)
        g.iterate()
        assert feed.empty()
        for p, k in enumerate(fams):
            msg = "%s, np = %d, population %d" % (FAMILIES[k], np_, p)
            assert g.get_state("evof", p)[0] == 1. and int(g.get_state("state", p)[0]) == 4, msg
            f = g.get_state("f", p)
            same_bits(f, want[p][1], msg)
            best, at = INF, -1
            for part in (f[:chunk], f):                # pso_gbest of the first chunk, pso_finish of the swarm
                i = first_min(part)
                if part[i] < best:
                    best, at = part[i], i
            same_bits(g.get_state("fbest", p), [best], msg)
            if at >= 0:
                x = g.get_state("x", p).reshape(np_, n)
                assert np.unique(x, axis=0).shape[0] == np_, msg
                same_bits(g.get_state("xbest", p), x[at], msg)


# ---- SLPSO -------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("np_", SLPSO_NP)
def test_slpso_initial_best_is_the_first_minimum(hip, np_):
    n = 2
    lo, hi = box(n)
    for P in (1, 3):
        for fams in groups(P):
            feed = Feed()
            out, want = [], []
            for k in fams:
                o, w = nan_first(family(k, np_))
                out.extend(o)
                want.append(w)
            feed.load(out)
            g = hip.SLPSO(10 ** 9, 0., np_, seed=14, populations=P)
            g.initialize(feed, lo, hi, np.zeros(P * n))
            assert feed.empty()
            for p, k in enumerate(fams):
                msg = "%s, np = %d, population %d" % (FAMILIES[k], np_, p)
                f = g.get_state("fx", p)
                same_bits(f, want[p], msg)
                i = first_min(f)
                same_bits(g.get_state("fabest", p), [f[i]], msg)
                same_bits(g.get_state("abest", p), g.get_state("x", p).reshape(np_, n)[i], msg)


# ---- CSO ---------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("P", [1, 3])
@pytest.mark.parametrize("np_,pc", CSO_CASES, ids=["np%d-pc%d" % c for c in CSO_CASES])
def test_cso_group_sort_is_stable_in_the_shuffled_order(hip, np_, pc, P):
    """the initial swarm through the callback (slot s is row s there), then a generation: every group of the
    shuffled slots is sorted by the values the swarm held, ties in the shuffled order.  The losers' new values
    (+inf) come after the sort."""
    n = 2
    lo, hi = box(n)
    for fams in groups(P):
        feed = Feed(rest=INF)
        out, want = [], []
        for k in fams:
            o, w = nan_first(family(k, np_))
            out.extend(o)
            want.append(w)
        feed.load(out)
        g = hip.CSO(10 ** 9, 0., np_, pcompete=pc, seed=15, populations=P)
        g.initialize(feed, lo, hi, np.zeros(P * n))
        assert feed.empty() and int(g.get_state("np")[0]) == np_
        for p in range(P):
            np.testing.assert_array_equal(ints(g.get_state("home", p)), np.arange(np_))
            same_bits(g.get_state("f", p), want[p])
        with pytest.raises(Exception):
            g.set_state("shuffled", np.arange(np_))              # read-only
        g.iterate()
        assert feed.calls == P * (np_ + np_ - np_ // pc)           # (the winners are not evaluated again)
        for p, k in enumerate(fams):
            msg = "%s, np = %d, pcompete = %d, population %d" % (FAMILIES[k], np_, pc, p)
            src, home = ints(g.get_state("shuffled", p)), ints(g.get_state("home", p))
            assert sorted(src) == list(range(np_)) and not np.array_equal(src, np.arange(np_)), msg
            f = want[p]
            ref = np.concatenate([s_[np.argsort(f[s_], kind="stable")] for s_ in src.reshape(np_ // pc, pc)])
            np.testing.assert_array_equal(home, ref, err_msg=msg)
