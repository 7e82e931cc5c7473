"""The culling step of the traversal engine (csrc/rt_wide_step.h), as oracle/wide_step_model.h restates it, against the definition it
serves -- on inputs placed AT the threshold (tests/wide_step_cases.py), where hit parity on scenes cannot look: both tests carry the
slack 1 + 2^-16, so a margin that is too small loses a hit only where the canonical lo / hi is within ulps of that number.

The header's claim: the canonical test (slab() of oracle/oracle_bvh.h) passes on the decoded box of a used slot => the step
keeps that slot.  Held here with zero exceptions; tests/test_gpu_wide_step.py holds the kernel to the model value for value.

The tests prove their own teeth: with the margin's 2^-20 set to 0 the implication breaks in every sub-family of the threshold sweeps, with
its 1e-37 set to 0 it breaks at the floor of the margin (family (c)) -- measured on these inputs: 567 items in 148 of 1138 sweeps, and 1211
items in 19 of 96 sweeps.  And the step may not get looser either: the share of slots it keeps although float64 rejects them is held to
tests/golden/wide_step_bounds.json (81644 of 587208; a tenfold margin: 202842)."""
import collections
import json

import numpy as np
import pytest

import wide_step_cases as C


@pytest.fixture(scope="module")
def cases(oracle):
    return C.build(oracle)


@pytest.fixture(scope="module")
def shipped(oracle, cases):
    return C.evaluate(oracle, cases)


def breaks(e):
    """items on which the canonical test passes on a used slot that the step culls"""
    return (e["canonical"] & e["used"] & ~e["kept"]).any(axis=1)


def test_the_cases_are_what_they_say(cases, shipped):
    fam = cases["families"]
    total = sum(f["index"].size for f in fam.values())
    assert cases["nodes"].shape[0] <= 300 and total <= 220000, (cases["nodes"].shape, total)
    # every sweep holds both canonical verdicts on the child it was placed for
    for name in ("a", "b", "c", "d", "e"):
        f, e = fam[name], shipped[name]
        ns = len(f["labels"])
        assert ns >= (1000 if name == "a" else 60), (name, ns)
        v = e["canonical"][:ns * (2 * C.HALF + 1)].reshape(ns, 2 * C.HALF + 1, 4)[np.arange(ns), :, f["child"]]
        assert np.all(v.any(axis=1) & ~v.all(axis=1)), name
    # (a): every listed origin, scale, octant, binding side and distance is there
    have = collections.Counter(l for lab in fam["a"]["labels"] for l in lab)
    want = ["origin0", "origin4000", "origin1e+06"] + ["scale2^%d" % s for s in C.A_SCALES] + ["oct%d" % o for o in range(8)] + ["planes", "tmin", "tbest", "near", "far"]
    assert all(have[w] >= 100 for w in want), have
    a = fam["a"]
    far = np.abs(a["O"][:, :3]).max(axis=1)
    assert far.min() < 1e-30 and far.max() > 1e7
    assert not shipped["a"]["model"]["steep"].any() and not shipped["c"]["model"]["steep"].any()      # (the margin path, all of them)
    # (b): the reciprocals reached: 65536 itself, the nearest float reciprocals either side (two ulps below: 1 / x skips one), 1e5, 1e9, +-inf
    with np.errstate(divide="ignore"):
        inv = np.abs(np.float32(1.0) / fam["b"]["D"][:, :3])
    for v in (65536.0, 65536.0 + 2.0 ** -7, 65536.0 - 2.0 ** -7, np.inf):
        assert (inv == np.float32(v)).any(), v
    assert (inv > 9.9e8).any() and ((inv > 9.9e4) & (inv < 1.1e5)).any() and np.signbit(fam["b"]["D"][:, :3][fam["b"]["D"][:, :3] == 0]).any()
    # (c): node origin 0, the smallest scale, ray origin 0 or denormal
    nc = cases["nodes"][fam["c"]["index"]].view(np.float32)
    assert np.all(nc[:, 0:3] == 0) and np.all(nc[:, [3, 10, 11]] == np.float32(2.0) ** -126) and np.abs(fam["c"]["O"][:, :3]).max() < 2.0 ** -126
    assert (fam["c"]["O"][:, :3] == 0).all(axis=1).any() and (fam["c"]["O"][:, :3] != 0).any()
    # (d), (e), (f)
    assert np.isinf(cases["nodes"][fam["d"]["index"]].view(np.float32)[:, [3, 10, 11]]).sum(axis=1).max() == 3
    assert (~shipped["e"]["used"]).any() and np.isnan(fam["f"]["O"]).any() and np.isinf(fam["f"]["D"]).any() and (fam["f"]["O"][:, 3] > fam["f"]["D"][:, 3]).any()


def test_canonical_hit_implies_the_step_keeps_the_slot(cases, shipped):
    for name, e in shipped.items():
        bad = np.nonzero(breaks(e))[0]
        f = cases["families"][name]
        assert bad.size == 0, "family %s: %d items; first: node %s origin %s direction %s" % (
            name, bad.size, cases["nodes"][f["index"][bad[0]]], f["O"][bad[0]], f["D"][bad[0]])


def test_steep_rays_get_the_canonical_test_itself(cases, shipped):
    n_steep = 0
    for name, e in shipped.items():
        D = cases["families"][name]["D"]
        with np.errstate(divide="ignore"):
            inv = np.abs(np.float32(1.0) / D[:, :3])
        steep = ~(np.fmax.reduce(inv, axis=1) <= np.float32(65536.0))
        assert np.array_equal(e["model"]["steep"], steep), name
        assert np.array_equal(e["kept"][steep], (e["canonical"] & e["used"])[steep]), name
        n_steep += int(steep.sum())
    assert n_steep > 10000


def test_unused_slots_order_and_pushes(cases, shipped):
    """what the step does with its verdicts, derived again from the mask and the entry distances: an unused slot is never kept; the closest-hit
    step enters the nearest kept child and pushes the others farthest first; the any-hit step enters the first kept slot and pushes the later
    ones, highest first"""
    inf = np.float32(np.inf)
    for name, e in shipped.items():
        m, code = e["model"], C.decode(cases["nodes"])["code"][cases["families"][name]["index"]]
        assert not (e["kept"] & ~e["used"]).any(), name
        dist = m["dist"]
        assert np.all((dist < inf) <= e["kept"]) and not np.isnan(dist).any(), name
        for mode, kept in (("closest", e["kept"] & (dist < inf)), ("anyhit", e["kept"])):
            out = m[mode]
            n_kept = kept.sum(axis=1)
            assert np.array_equal(out[:, 1], np.maximum(n_kept - 1, 0)), (name, mode)
            assert np.array_equal(out[:, 0] == C.EMPTY, n_kept == 0), (name, mode)
            seq = np.concatenate([out[:, 0:1], out[:, 2:5][:, ::-1]], axis=1)            # the node entered, then rows 2 1 0: the order they pop in
            for i in np.nonzero(n_kept > 0)[0][:: max(1, int((n_kept > 0).sum()) // 4000)]:
                order = [c for c in seq[i] if c != C.NONE]
                slots = [int(np.nonzero(code[i] == c)[0][0]) for c in order]
                assert sorted(slots) == list(np.nonzero(kept[i])[0]), (name, mode, i)
                if mode == "closest":
                    assert np.all(np.diff(dist[i, slots]) >= 0), (name, mode, i)
                else:
                    assert slots == sorted(slots), (name, mode, i)


def test_teeth_no_margin_breaks_every_subfamily_of_the_sweeps(oracle, cases):
    e = C.evaluate(oracle, dict(nodes=cases["nodes"], families={"a": cases["families"]["a"]}), margin_scale=0.0)["a"]
    f = cases["families"]["a"]
    ns = len(f["labels"])
    broken = breaks(e).reshape(ns, -1).any(axis=1)
    count, of = collections.Counter(), collections.Counter()
    for s, lab in enumerate(f["labels"]):
        for l in lab:
            of[l] += 1
            count[l] += int(broken[s])
    print("margin_scale = 0: %d items in %d of %d sweeps; sweeps broken per sub-family: %s" % (
        int(breaks(e).sum()), int(broken.sum()), ns, {l: "%d/%d" % (count[l], of[l]) for l in sorted(of)}))
    assert all(count[l] >= 1 for l in of), {l: count[l] for l in of if count[l] == 0}


def test_teeth_no_floor_breaks_the_margin_floor_family(oracle, cases):
    e = C.evaluate(oracle, dict(nodes=cases["nodes"], families={"c": cases["families"]["c"]}), tiny=0.0)["c"]
    ns = len(cases["families"]["c"]["labels"])
    print("tiny = 0: %d items in %d of %d sweeps of family (c)" % (int(breaks(e).sum()), int(breaks(e).reshape(ns, -1).any(axis=1).sum()), ns))
    assert breaks(e).any()


def test_the_step_is_no_looser_than_measured(oracle, cases):
    with open(C.GOLDEN) as fh:
        bound = json.load(fh)["family_a"]
    a = cases["families"]["a"]
    loose, slots = C.looseness(oracle, cases["nodes"], a)
    print("family (a): the step keeps %d of %d used slots that float64 rejects (bound %d of %d)" % (loose, slots, bound["kept_but_rejected_in_float64"], bound["slots"]))
    assert slots == bound["slots"] and a["index"].size == bound["items"], "the cases changed: python tests/wide_step_cases.py --write"
    assert loose <= bound["kept_but_rejected_in_float64"]
    # ... which a tenfold margin exceeds, and a sixteenth of the margin stays far below (and breaks the implication, above)
    assert C.looseness(oracle, cases["nodes"], a, margin_scale=10 * 2.0 ** -20)[0] > 2 * bound["kept_but_rejected_in_float64"]
    assert C.looseness(oracle, cases["nodes"], a, margin_scale=2.0 ** -24)[0] < bound["kept_but_rejected_in_float64"] // 2
