"""ONE step of the traversal engine on the GPU (rt_debug_wide_step: the wide_step template the trace kernels call, csrc/rt_wide_step.h)
against its restatement oracle/wide_step_model.h, value for value -- the node entered, the stack pointer, the rows pushed in order -- for
the closest-hit and the any-hit step, the pure-LDS and the DEEP instantiation, nodes read from the LDS-resident top and from global memory.

The inputs are the enumerated cases of tests/wide_step_cases.py, on which tests/test_wide_step_edges.py holds the model to the canonical
box test (canonical passes on the decoded box => the step keeps the slot), and the same threshold sweeps against the children of nodes
sampled from trees the builder made.  Mutations of the step, each run once on a scratch build, all fail here (items that differ from
the model: DESIGN.md section 6): margin 0, 2^-20 -> 2^-24, 2^-20 -> 2^-16, 65536 -> 1e30, near / far bytes swapped on one axis, one exchange
of the sort removed, + 1e-37 dropped."""
import numpy as np
import pytest

import wide_step_cases as C
import wide_tree as W
from util import HARD_FAMILIES, hard_xforms, triangle_soup

pytestmark = pytest.mark.gpu

VARIANTS = [(anyhit, deep, lds_top) for anyhit in (False, True) for deep in (False, True) for lds_top in (False, True)]


@pytest.fixture(scope="module")
def four_wide(capi):
    assert capi.wide_layout() == (4, 64), "the one-step entry and its model are the four-wide step's"


@pytest.fixture(scope="module")
def cases(oracle):
    c = C.build(oracle)
    fam = c["families"].values()
    c["index"] = np.concatenate([f["index"] for f in fam])
    c["O"] = np.concatenate([f["O"] for f in fam])
    c["D"] = np.concatenate([f["D"] for f in fam])
    c["model"] = oracle.wide_step_model(c["nodes"], c["index"], c["O"], c["D"])
    return c


def assert_parity(gpu, nodes, index, O, D, model, what):
    for anyhit, deep, lds_top in VARIANTS:
        got = gpu.wide_step(nodes, index, O, D, anyhit=anyhit, deep=deep, lds_top=lds_top)
        want = model["anyhit" if anyhit else "closest"]
        bad = np.nonzero((got != want).any(axis=1))[0]
        assert bad.size == 0, "%s, anyhit %d deep %d lds_top %d: %d of %d items differ; first %d: node %s origin %s direction %s: GPU %s model %s" % (
            what, anyhit, deep, lds_top, bad.size, index.size, bad[0], nodes[index[bad[0]]], O[bad[0]], D[bad[0]], got[bad[0]], want[bad[0]])


def test_enumerated_cases(gpu, capi, four_wide, cases):
    assert_parity(gpu, cases["nodes"], cases["index"], cases["O"], cases["D"], cases["model"], "enumerated cases")


def test_bad_arguments_are_errors(gpu, capi, four_wide, cases):
    nodes, O, D = cases["nodes"], cases["O"][:4], cases["D"][:4]
    for index in ([0, 1, 2, nodes.shape[0]], [0, -1, 2, 3]):
        with pytest.raises(capi.RtError):
            gpu.wide_step(nodes, index, O, D)
    with pytest.raises(capi.RtError):
        capi._check(capi.lib().rt_debug_wide_step(gpu.h, capi._ptr(np.zeros((129, 16), np.uint32)), 129, capi._ptr(np.zeros(1, np.int32)),
                                                  capi._ptr(O), capi._ptr(D), 1, capi.WIDE_STEP_LDS_TOP, capi._ptr(np.zeros(5, np.int32))))


def sweeps_on_tree(oracle, nodes, seed, n_sample=200, per_node=6):
    """family (a) of wide_step_cases against the decoded children of n_sample nodes of a tree, at the canonical and at the model's threshold"""
    r = np.random.default_rng(seed)
    dec = C.decode(nodes)
    pick = np.sort(r.choice(nodes.shape[0], min(n_sample, nodes.shape[0]), replace=False))
    sp = C.Specs()
    C.graze_specs_for(dec, pick, r, sp, lambda ni: (), per_node)
    a = C.place_sweeps(sp, C.canonical_verdict(oracle, dec), C.HALF)
    b = C.place_sweeps(sp, C.model_verdict(oracle, nodes), C.HALF_MODEL)
    assert a["placed"] >= len(sp.node) // 2 and b["placed"] >= len(sp.node) // 2, (a["placed"], b["placed"], len(sp.node))
    index, O, D = (np.concatenate([a[k], b[k]]) for k in ("index", "O", "D"))
    model = oracle.wide_step_model(nodes, index, O, D)
    kept = (model["mask"][:, None] >> np.arange(4)) & 1 != 0
    used = dec["code"][index] != C.NONE
    assert not (C.canonical(oracle, dec, index, O, D) & used & ~kept).any(), "the canonical test passes on a slot the step culls"
    return index, O, D, model


def test_blas_of_a_shifted_soup(gpu, capi, oracle, four_wide):
    v, i = triangle_soup(4000, seed=77)
    v["position"] += np.array([4000.0, -2500.0, 3000.0], np.float32)
    sc = capi.Scene(gpu)
    sc.add_model(capi.Model(gpu, v, i), None)
    sc.build()
    st, nodes, root = W.check_blas(sc, 0, v, i)                 # the decoded boxes contain their subtrees
    assert st["nodes"] > 500
    index, O, D, model = sweeps_on_tree(oracle, nodes, seed=1)
    assert_parity(gpu, nodes, index, O, D, model, "BLAS of the shifted soup")


def test_tlas_of_hard_instances(gpu, capi, oracle, four_wide):
    v, i = triangle_soup(300, seed=78, extent=2.0, size=0.4)
    xf = np.concatenate([hard_xforms(f, 6, seed=21 + k) for k, f in enumerate(HARD_FAMILIES)])[:40]
    sc = capi.Scene(gpu)
    m = capi.Model(gpu, v, i)
    for x in xf:
        sc.add_model(m, x)
    sc.build()
    nodes, root, _ = sc.wide_read(-1)
    boxes = np.stack([sc.instance_info(k)[0] for k in range(40)])
    W.check(nodes, root, boxes[:, :3], boxes[:, 3:], 40, blas=False)
    index, O, D, model = sweeps_on_tree(oracle, nodes, seed=2, per_node=48)
    assert_parity(gpu, nodes, index, O, D, model, "TLAS of 40 hard instances")
