"""--clique-gradient / --unbiased-gradient under --device-training, the parts that need no GPU:
what check_eligible accepts and refuses, the clique segments the trainer hands to the fused mean +
step kernel, the C entry point's argument checks, and header, ctypes table and torch op agreeing."""
import os
import re

import numpy as np
import pytest
import torch

from conftest import REPO
from test_train_host import _nodes, _params

FLAGS = {"device-training": {}, "device-training-gn-lenet": {"device-training-gn-lenet": True}}
N = 6
CLIQUES = [[0, 1, 2], [4, 3]]                      # node 5 is in none
EDGES = {0: [1, 2], 1: [0, 2], 2: [0, 1, 3], 3: [2, 4], 4: [3, 5], 5: [4]}
HOODS = {0: [0, 1], 1: [1, 0, 2], 2: [2], 3: [3, 2, 4, 5], 4: [4, 3], 5: [5, 4]}


def _topo(**extra):
    t = {"edges": EDGES, "cliques": CLIQUES, "neighbourhoods": HOODS}
    t.update(extra)
    return t


@pytest.mark.parametrize("flag", list(FLAGS))
@pytest.mark.parametrize("avg", ["clique-gradient", "unbiased-gradient", "both"])
def test_check_eligible_accepts_gradient_averaging(flag, avg):
    """With a topology that gives the averaging lists, both flags are accepted and the shape tuple
    is the one returned without them; d_sgd.init passes its topology on."""
    from niidmix import d_sgd, train
    on = {"clique-gradient": True, "unbiased-gradient": True} if avg == "both" else {avg: True}
    plain, p = _params(**FLAGS[flag]), _params(**FLAGS[flag], **on)
    nodes = _nodes(p, n=N)
    assert train.check_eligible(nodes, p, _topo()) == train.check_eligible(nodes, plain) == (6, 3)
    state, _, _ = d_sgd.init(nodes, _topo(), p)
    assert state["step"] == 0
    # clique wins when both are set, as in the reference: no 'neighbourhoods' needed then
    if avg == "both":
        t = _topo()
        del t["neighbourhoods"]
        assert train.check_eligible(nodes, p, t) == (6, 3)
        assert train.grad_plan(N, t, p, "x").kind == "clique"


@pytest.mark.parametrize("flag", list(FLAGS))
def test_refusals_name_the_flag(flag):
    from niidmix import train
    cg, ug = {"clique-gradient": True}, {"unbiased-gradient": True}

    def refused(on, topo):
        p = _params(**FLAGS[flag], **on)
        with pytest.raises(ValueError, match=flag):
            train.check_eligible(_nodes(p, n=N), p, topo)

    for on in (cg, ug):
        refused(on, None)                                            # no topology at all
        refused(on, {"edges": EDGES})                                # lacks its key
    refused(cg, {"edges": EDGES, "neighbourhoods": HOODS})           # the other flag's key
    refused(ug, {"edges": EDGES, "cliques": CLIQUES})
    refused(cg, _topo(cliques=[[0, 1, 2], [2, 3]]))                  # overlapping cliques
    refused(cg, _topo(cliques=[[0, 1], [4, N]]))                     # member out of range
    refused(cg, _topo(cliques=[[0, -1]]))
    refused(ug, _topo(neighbourhoods={**HOODS, 2: []}))        # empty neighbourhood
    refused(ug, _topo(neighbourhoods={**HOODS, 2: [2, N]}))    # member out of range
    refused(ug, _topo(neighbourhoods={r: HOODS[r] for r in range(N - 1)}))   # a node without one
    p = _params(**FLAGS[flag], **cg)
    p["topology"]["remove-clique-edges"] = 1
    with pytest.raises(ValueError, match=flag):                      # removed edges need 'edges'
        train.check_eligible(_nodes(p, n=N), p, {"cliques": CLIQUES})


@pytest.mark.parametrize("flag", list(FLAGS))
def test_sample_topology_is_still_refused(flag):
    from niidmix import train
    for on in ({}, {"clique-gradient": True}, {"unbiased-gradient": True}):
        p = _params(**FLAGS[flag], **on)
        p["topology"]["name"] = "sample"
        with pytest.raises(ValueError, match="'sample' topology"):
            train.check_eligible(_nodes(p, n=N), p, _topo())


def test_clique_segments_exclude_loners():
    """build_grad_plan gives every node in no clique a one-member segment; the trainer's fused
    mean + step must not see those (the reference does not step such a node)."""
    from niidmix import train
    from niidmix.gradient import build_grad_plan
    params = {"algorithm": {"clique-gradient": True}, "topology": {"remove-clique-edges": 0}}
    cliques = [[3, 1], [7, 6, 5], [8]]                      # 0, 2, 4 and 9 are in none
    plan = build_grad_plan(10, {"cliques": cliques}, params)
    assert len(plan.seg_ptr) - 1 == 3 + 4 and plan.stepped == [3, 1, 7, 6, 5, 8]
    seg_ptr, seg_row = train.clique_segments(plan)
    assert seg_ptr.dtype == np.int32 and seg_row.dtype == np.int32
    assert seg_ptr.tolist() == [0, 2, 5, 6] and seg_row.tolist() == [3, 1, 7, 6, 5, 8]
    seg_row[0] = 99                                         # copies: the plan is left alone
    assert plan.seg_row[0] == 3
    # every node in a clique: nothing to drop; no clique at all: no segment
    full = build_grad_plan(4, {"cliques": [[1, 0], [2, 3]]}, params)
    assert [a.tolist() for a in train.clique_segments(full)] == [[0, 2, 4], [1, 0, 2, 3]]
    none = build_grad_plan(3, {"cliques": []}, params)
    assert [a.tolist() for a in train.clique_segments(none)] == [[0], []]


def test_fused_step_argument_errors_without_gpu():
    """Validation happens before any HIP call, so the documented codes come back on a CPU-only
    host too (the made-up addresses are never dereferenced)."""
    from niidmix import _lib
    L = _lib.lib
    F = L.niidmix_grad_segment_mean_sgd_step_f32
    base, far, far2 = 1 << 20, 1 << 30, 1 << 31

    def call(p=base, ld_p=8, g=far, ld_g=8, buf=far2, ld_b=8, ncols=8, n_seg=2, seg_ptr=8,
             seg_row=8, n_members=4, momentum=0.9, first=0):
        return F(p, ld_p, g, ld_g, buf, ld_b, ncols, n_seg, seg_ptr, seg_row, n_members, -0.1,
                 momentum, first, None)

    def err():
        return L.niidmix_last_error()

    for name in ("ncols", "n_seg", "n_members"):
        assert call(**{name: -1}) == _lib.EINVAL and b"negative" in err(), name
    for name in ("ncols", "n_seg", "n_members"):                       # empty before null
        assert call(**{name: 0}, p=None, g=None, buf=None, seg_ptr=None, seg_row=None) == _lib.OK
    for name in ("p", "g", "buf", "seg_ptr", "seg_row"):
        assert call(**{name: None}) == _lib.EINVAL and b"null" in err(), name
    # buf is exempt only without momentum (then its leading dimension is not looked at either)
    assert call(buf=None, ld_b=0, momentum=0.0, ld_p=7) == _lib.EINVAL and b"leading" in err()
    assert call(buf=None, momentum=0.9, first=1) == _lib.EINVAL and b"null" in err()
    assert call(p=None, ld_p=2) == _lib.EINVAL and b"null" in err()                 # null before ld
    for name in ("ld_p", "ld_g", "ld_b"):
        assert call(**{name: 7}) == _lib.EINVAL and b"leading dimension < ncols" in err(), name
    assert call(ld_p=7, g=base) == _lib.EINVAL and b"leading" in err()              # ld before alias
    # any two of p, g, buf over (n_members - 1) * ld + ncols = 32 elements
    assert call(g=base + 4 * 20) == _lib.EALIAS and b"p and g" in err()
    assert call(buf=base + 4 * 20, first=1) == _lib.EALIAS and b"p and buf" in err()
    assert call(p=far + 4 * 31, buf=far2) == _lib.EALIAS and b"p and g" in err()
    assert call(buf=far + 4 * 20) == _lib.EALIAS and b"g and buf" in err()
    assert call(p=base, g=base, buf=base) == _lib.EALIAS and b"p and g" in err()
    assert call(g=base + 4 * 20, momentum=0.0, buf=None, ld_b=0) == _lib.EALIAS
    assert call(ncols=0, g=base) == _lib.OK                                         # empty before alias


def test_header_table_and_op_agree():
    from niidmix import _lib, ops  # noqa: F401  (registers the op)
    text = open(os.path.join(REPO, "include", "niidmix.h")).read()
    m = re.search(r"^int niidmix_grad_segment_mean_sgd_step_f32\(([^)]*)\);", text, re.M)
    assert m and "#define NIIDMIX_ABI_VERSION 6" in text and _lib.lib.niidmix_abi_version() == 6
    args = [" ".join(a.split()) for a in m.group(1).split(",")]
    assert args == ["float *p", "int64_t ld_p", "const float *g", "int64_t ld_g", "float *buf",
                    "int64_t ld_b", "int64_t ncols", "int64_t n_seg", "const int32_t *seg_ptr",
                    "const int32_t *seg_row", "int64_t n_members", "float neg_lr", "float momentum",
                    "int first", "void *stream"]
    import ctypes
    res, sig = _lib.SIGNATURES["niidmix_grad_segment_mean_sgd_step_f32"]
    kinds = {"int64_t": ctypes.c_int64, "float": ctypes.c_float, "int": ctypes.c_int}
    want = [ctypes.c_void_p if "*" in a else kinds[a.split()[0]] for a in args]
    assert res is ctypes.c_int and sig == want
    schema = str(torch.ops.niidmix.grad_segment_mean_sgd_step.default._schema)
    assert re.sub(r"\(a\d!\)", "(!)", schema) == (
        "niidmix::grad_segment_mean_sgd_step(Tensor(!) p, Tensor g, Tensor(!)? buf, Tensor seg_ptr, "
        "Tensor seg_row, float neg_lr, float momentum, bool first) -> ()")
    # no CPU fallback: host tensors are refused before the library is called
    z, i = torch.zeros(2, 4), torch.zeros(2, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="HIP"):
        torch.ops.niidmix.grad_segment_mean_sgd_step(z, z.clone(), None, i, i, -0.1, 0.0, False)
