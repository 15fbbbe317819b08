"""--clique-gradient / --unbiased-gradient under --device-training on the GPU: the fused segment
mean + SGD step kernel bit for bit against its two-launch composition and against the reference's
CPU arithmetic, and the trainer's rounds put together from their parts.

References of the kernel tests:
  (a) niidmix::grad_segment_mean followed by niidmix::sgd_step_rows / sgd_momentum_step_rows over
      the member rows, on the same inputs;
  (b) torch on the CPU: d_sgd.average_gradients / update_gradients on one parameter tensor per
      row, then torch.optim.SGD(lr, momentum).step() (the reference's d_sgd.gradient, :56-65).
"""
import pytest
import torch
import torch.nn.functional as F

import test_eval_gnlenet_host as th

pytestmark = pytest.mark.gpu

ROWS, LR, MOM, SENT = 140, 0.07, 0.9, 12345.678
NCOLS = [1, 5, 1023, 1024, 1028, 2052]      # V = 1 and V = 4, the chunk edges at 256 and 1024


def _segments(which):
    """'mixed': lengths 64 (odd rows 13..139, interleaved with the 63), 1, 0, 9 (reversed), 63, 2
    over rows 1..139, row 0 in none.  'long': one segment of 130 members (64 + 64 + 2: a second and
    a third descriptor fetch and the U-tail), rows 5..134 shuffled."""
    if which == "mixed":
        return [list(range(13, 140, 2)), [1], [], list(range(12, 3, -1)), list(range(14, 139, 2)),
                [2, 3]]
    perm = torch.randperm(130, generator=torch.Generator().manual_seed(77)).tolist()
    return [[5 + v for v in perm]]


class Row(torch.nn.Module):
    def __init__(self, v):
        super().__init__()
        self.w = torch.nn.Parameter(v.clone())


_cache = {}


def _case(ncols, which, momentum, poison=False):
    """Inputs of three consecutive steps and reference (b), computed once: p0 [ROWS, ncols], g
    [3, ROWS, ncols], and per step the CPU parameters and momentum buffers of the member rows."""
    from niidmix import d_sgd
    key = (ncols, which, momentum, poison)
    if key in _cache:
        return _cache[key]
    segs = _segments(which)
    members = [r for s in segs for r in s]
    gen = torch.Generator().manual_seed(1000 * ncols + len(members))
    p0 = torch.randn(ROWS, ncols, generator=gen)
    g = torch.randn(3, ROWS, ncols, generator=gen)
    # signed zeros: a whole segment's gradients -0.0 (its mean is +0: zeros_like + add_), one
    # member's alone, and parameters
    g[:, members[-2:], 0] = -0.0
    g[1, members[0], ncols - 1] = -0.0
    p0[members[-1], 0] = -0.0
    p0[members[3 % len(members)], ncols // 2] = -0.0
    if poison:
        g[0, members[70], 7], g[0, members[70], 600] = float("inf"), float("nan")
    rows = {r: Row(p0[r]) for r in members}
    opts = {r: torch.optim.SGD(rows[r].parameters(), lr=LR, momentum=momentum) for r in members}
    want = []
    for step in range(3):
        for r in members:
            rows[r].w.grad = g[step, r].clone()
        for s in segs:
            models = [rows[r] for r in s]
            if models:
                d_sgd.update_gradients(models, d_sgd.average_gradients(models))
                for r in s:
                    opts[r].step()
        pw = torch.stack([rows[r].w.detach().clone() for r in members])
        bw = torch.stack([opts[r].state[rows[r].w]["momentum_buffer"].clone() for r in members]) \
            if momentum else None
        want.append((pw, bw))
    out = dict(segs=segs, members=members, p0=p0, g=g, want=want)
    _cache[key] = out
    return out


def _slab(values, members, ncols, dev):
    """[ROWS, padded + 8] of sentinels with `values` in the member rows' first ncols columns."""
    ld = (ncols + 3) // 4 * 4 + 8
    s = torch.full((ROWS, ld), SENT)
    if values is not None:
        s[members, :ncols] = values[members]
    return s.to(dev)


def _descr(segs, dev):
    ptr = [0]
    for s in segs:
        ptr.append(ptr[-1] + len(s))
    return (torch.tensor(ptr, dtype=torch.int32, device=dev),
            torch.tensor([r for s in segs for r in s], dtype=torch.int32, device=dev))


def _bits(t):
    return t.contiguous().view(torch.int32)


def _run(d, ncols, momentum, dev, fused, steps=3):
    """The three steps on the device, fused or as composition (a).  Returns per step the whole p
    and buf slabs (CPU) and the g slab of the last step."""
    members = d["members"]
    seg_ptr, seg_row = _descr(d["segs"], dev)
    rows = seg_row.clone()
    p = _slab(d["p0"], members, ncols, dev)
    buf = _slab(None, members, ncols, dev) if momentum else None
    out = []
    for step in range(steps):
        g = _slab(d["g"][step], members, ncols, dev)
        pv, gv = p[:, :ncols], g[:, :ncols]
        bv = buf[:, :ncols] if momentum else None
        if fused:
            torch.ops.niidmix.grad_segment_mean_sgd_step(pv, gv, bv, seg_ptr, seg_row, -LR, momentum,
                                                         step == 0)
        else:
            avg = _slab(None, members, ncols, dev)
            torch.ops.niidmix.grad_segment_mean(gv, seg_ptr, seg_row, avg[:, :ncols])
            if momentum:
                torch.ops.niidmix.sgd_momentum_step_rows(pv, avg[:, :ncols], bv, rows, -LR, momentum,
                                                         step == 0)
            else:
                torch.ops.niidmix.sgd_step_rows(pv, avg[:, :ncols], rows, -LR)
        torch.cuda.synchronize()
        out.append((p.cpu(), buf.cpu() if momentum else None, g.cpu()))
    return out


@pytest.mark.parametrize("momentum", [0.0, MOM])
@pytest.mark.parametrize("which", ["mixed", "long"])
@pytest.mark.parametrize("ncols", NCOLS)
def test_fused_kernel_bitwise(ncols, which, momentum, gpu):
    """Three consecutive steps (momentum 0; momentum 0.9 with first = 1, 0, 0): p and buf equal
    (a) over the whole slab and (b) on the member rows, bit for bit; pad columns, rows in no
    segment (row 0 among them) and g keep their bits."""
    from niidmix import ops  # noqa: F401  (registers the ops)
    d = _case(ncols, which, momentum)
    members = d["members"]
    got = _run(d, ncols, momentum, gpu, fused=True)
    parts = _run(d, ncols, momentum, gpu, fused=False)
    others = [r for r in range(ROWS) if r not in set(members)]
    assert 0 in others
    for step in range(3):
        (p, buf, g), (pa, ba, _), (pw, bw) = got[step], parts[step], d["want"][step]
        assert torch.equal(_bits(p), _bits(pa)), f"step {step}: p differs from the two launches"
        assert torch.equal(_bits(p[members, :ncols]), _bits(pw)), f"step {step}: p differs from torch"
        for s in (p, buf) if momentum else (p,):
            assert bool((s[:, ncols:] == torch.tensor(SENT)).all()), "pad columns written"
            assert bool((s[others] == torch.tensor(SENT)).all()), "a row in no segment written"
        if momentum:
            assert torch.equal(_bits(buf), _bits(ba)), f"step {step}: buf differs from the two launches"
            assert torch.equal(_bits(buf[members, :ncols]), _bits(bw)), f"step {step}: buf differs from torch"
        assert torch.equal(_bits(g), _bits(_slab(d["g"][step], members, ncols, "cpu"))), "g written"


def test_empty_calls_are_no_ops(gpu):
    from niidmix import ops  # noqa: F401
    p = torch.full((4, 8), SENT, device=gpu)
    g = torch.ones(4, 8, device=gpu)
    zero = torch.zeros(1, dtype=torch.int32, device=gpu)
    none = torch.zeros(0, dtype=torch.int32, device=gpu)
    torch.ops.niidmix.grad_segment_mean_sgd_step(p, g, None, zero, none, -LR, 0.0, False)      # n_seg 0
    torch.ops.niidmix.grad_segment_mean_sgd_step(p, g, None, torch.zeros(3, dtype=torch.int32, device=gpu),
                                                 none, -LR, 0.0, False)                      # empty ones
    torch.cuda.synchronize()
    assert bool((p == SENT).all())
    with pytest.raises(RuntimeError, match="buf"):
        torch.ops.niidmix.grad_segment_mean_sgd_step(p, g, None, zero, none, -LR, MOM, True)
    two = torch.tensor([0, 2], dtype=torch.int32, device=gpu)
    with pytest.raises(RuntimeError, match="overlap"):                                       # g is p
        torch.ops.niidmix.grad_segment_mean_sgd_step(p, p, None, two, two, -LR, 0.0, False)
    assert bool((p == SENT).all())


def test_nan_containment(gpu):
    """An inf and a NaN in one member's gradient (columns 7 and 600, first step, momentum 0.9):
    after each of three steps every member of that segment is non-finite in those columns,
    exactly as in (b) -- the same bits, a NaN where (b) has a NaN (its payload is not compared) --
    and every other element has the clean run's bits."""
    from niidmix import ops  # noqa: F401
    ncols = 1028
    clean, d = _case(ncols, "mixed", MOM), _case(ncols, "mixed", MOM, poison=True)
    members = d["members"]
    bad_row = members[70]
    seg = next(s for s in d["segs"] if bad_row in s)
    got, ref = _run(d, ncols, MOM, gpu, fused=True), _run(clean, ncols, MOM, gpu, fused=True)
    hit = torch.zeros(ROWS, ncols, dtype=torch.bool)
    for c in (7, 600):
        hit[seg, c] = True
    for step in range(3):
        for k in (0, 1):                                             # p, then buf
            t, t_clean, want = got[step][k][:, :ncols], ref[step][k][:, :ncols], d["want"][step][k]
            assert not bool(torch.isfinite(t[hit]).any())
            assert torch.equal(_bits(t[~hit]), _bits(t_clean[~hit]))
            tm = t[members]
            assert torch.equal(torch.isnan(tm), torch.isnan(want))
            assert torch.equal(_bits(tm[~torch.isnan(tm)]), _bits(want[~torch.isnan(want)]))
    assert bool(torch.isinf(got[0][0][seg, 7]).all()) and bool(torch.isnan(got[0][0][seg, 600]).all())


def test_two_calls_give_the_same_bits(gpu):
    from niidmix import ops  # noqa: F401
    for ncols, momentum in ((2052, MOM), (1023, 0.0)):
        d = _case(ncols, "long", momentum)
        a, b = _run(d, ncols, momentum, gpu, True), _run(d, ncols, momentum, gpu, True)
        for (pa, ba, _), (pb, bb, _) in zip(a, b):
            assert torch.equal(_bits(pa), _bits(pb))
            assert ba is None or torch.equal(_bits(ba), _bits(bb))


# ------------------------------------------------------------------------------------------------
# the plugin's rounds
def _mh(edges, n):
    """Metropolis-Hastings weights: W[i, j] = 1 / (max(deg i, deg j) + 1), the rest on the diagonal."""
    w = torch.zeros(n, n)
    for i in range(n):
        for j in edges[i]:
            w[i, j] = 1.0 / (max(len(edges[i]), len(edges[j])) + 1)
    for i in range(n):
        w[i, i] = 1.0 - float(w[i].sum())
    return w


def _graph(cliques, links, n, drop=()):
    """Full cliques plus the `links` between them, minus the edges in `drop`."""
    pairs = {(a, b) for c in cliques for a in c for b in c if a != b}
    pairs |= {(a, b) for a, b in links} | {(b, a) for a, b in links}
    pairs -= {(a, b) for a, b in drop} | {(b, a) for a, b in drop}
    edges = {i: sorted(b for a, b in pairs if a == i) for i in range(n)}
    return edges


class Linear(torch.nn.Module):
    K, C = 51, 5                             # P = 260: the float4 path; GN-LeNet's P is odd

    def __init__(self):
        super().__init__()
        self.fc = torch.nn.Linear(self.K, self.C)

    def forward(self, x, params):
        return F.log_softmax(self.fc(x.view(-1, self.K)), dim=1)


class GNNet(th.GNLeNet):
    SHAPE = (1, 15, 15, 3)                   # the smallest samples of tests/test_gpu_train_gnlenet.py

    def __init__(self):
        super().__init__(self.SHAPE[0], self.SHAPE[3], self.SHAPE[1:3], 2)


LIN = dict(n=12, b=8, s=24, lr=0.1, cliques=[[0, 1, 2, 3], [7, 6, 5, 4], [8, 9, 10]],
           links=[(3, 4), (7, 8), (10, 11), (11, 0)], model="linear", seed=2024, data_seed=99)
# models and samples of tests/test_gpu_train_gnlenet.py's rounds (its seeds), batch 2
GN = dict(n=4, b=2, s=12, lr=0.05, cliques=[[0, 1], [3, 2]], links=[(1, 2), (3, 0)], model="gn",
          seed=2025, data_seed=314)
_data = {}


def _dataset(cfg):
    name = cfg["model"]
    if name not in _data:
        g = torch.Generator().manual_seed(cfg["data_seed"])
        m = cfg["n"] * cfg["s"]
        if name == "linear":
            x = torch.rand(m, Linear.K, generator=g) * (torch.rand(m, Linear.K, generator=g) < 0.5)
            y = (x @ torch.randn(Linear.K, Linear.C, generator=g)).argmax(1)
        else:
            x = torch.randn(m, *GNNet.SHAPE[:3], generator=g)
            y = torch.randint(0, GNNet.SHAPE[3], (m,), generator=g)
        _data[name] = (x, y)
    return _data[name]


def _setup(cfg, device_training=True, momentum=0.0, avg="clique-gradient", removed=False):
    from niidmix import d_sgd
    torch.manual_seed(cfg["seed"])
    n, s = cfg["n"], cfg["s"]
    params = {"meta": {"log": "WARNING", "seed": cfg["seed"]}, "nodes": {"nb-nodes": n},
              "topology": {"name": "d-cliques", "remove-clique-edges": 1 if removed else 0},
              "logger": {"accuracy-logging-interval": 0, "accuracy-logging-interval-steps": 0,
                         "log-consensus-distance": False},
              "algorithm": {"learning-rate": cfg["lr"], "learning-momentum": momentum,
                            "batch-size": cfg["b"], "initial-averaging": False,
                            "clique-gradient": avg == "clique-gradient",
                            "unbiased-gradient": avg == "unbiased-gradient",
                            "deferred-writeback": False, "mixing-mode": "exact"}}
    if device_training:
        params["algorithm"]["device-training"] = True
        if cfg["model"] == "gn":
            params["algorithm"]["device-training-gn-lenet"] = True
    x, y = _dataset(cfg)
    gen = torch.Generator().manual_seed(2026)
    nodes = []
    for r in range(n):
        mdl = Linear() if cfg["model"] == "linear" else th.perturb(GNNet(), gen)
        ts = [(x[r * s + j], int(y[r * s + j])) for j in range(s)]
        nodes.append({"rank": r, "epoch": 0, "train-set": ts, "model": mdl,
                      "optimizer": d_sgd.optimizer(mdl, params)})
    edges = _graph(cfg["cliques"], cfg["links"], n, drop=[(0, 2)] if removed else ())
    topo = {"edges": edges, "weights": _mh(edges, n), "cliques": cfg["cliques"]}
    if avg == "unbiased-gradient":          # unequal lengths, the node itself not always first
        topo["neighbourhoods"] = {r: (edges[r] + [r] if r % 2 else [r] + edges[r][::-1])
                                  for r in range(n)}
    state, _, _ = d_sgd.init(nodes, topo, params)
    return params, nodes, topo, state


def _flat(nodes):
    return torch.stack([torch.cat([q.detach().reshape(-1) for q in nd["model"].parameters()])
                        for nd in nodes]).clone()


def _reference_gradient(nodes, topo, params):
    """The reference's d_sgd.gradient (:47-94) on the CPU with the plugin's own average_gradients /
    update_gradients and the nodes' torch.optim.SGD optimizers."""
    from niidmix import d_sgd
    alg = params["algorithm"]
    if alg["clique-gradient"] and not params["topology"]["remove-clique-edges"]:
        for clique in topo["cliques"]:
            models = [nodes[r]["model"] for r in clique]
            d_sgd.update_gradients(models, d_sgd.average_gradients(models))
            for r in clique:
                nodes[r]["optimizer"].step()
    elif alg["clique-gradient"]:
        for clique in topo["cliques"]:
            means = {r: d_sgd.average_gradients([nodes[q]["model"] for q in clique
                                                 if q == r or q in topo["edges"][r]]) for r in clique}
            for r in clique:
                d_sgd.update_gradients([nodes[r]["model"]], means[r])
                nodes[r]["optimizer"].step()
    else:
        means = {nd["rank"]: d_sgd.average_gradients([nodes[q]["model"]
                                                      for q in topo["neighbourhoods"][nd["rank"]]])
                 for nd in nodes}
        for nd in nodes:
            d_sgd.update_gradients([nd["model"]], means[nd["rank"]])
            nd["optimizer"].step()


def _parts_round(cfg, batches, topo, nodes, params, dev, oracle_mod):
    """mix(step(mean(g_kernel))): the gradient op on the same indices, the reference's gradient
    averaging and optimizer steps on the CPU, the oracle's reference loop for the mixing."""
    from niidmix import train
    n, b, s = cfg["n"], cfg["b"], cfg["s"]
    x, y = _dataset(cfg)
    theta = _flat(nodes)
    p = theta.shape[1]
    tht = torch.zeros(n, train.padded_ld(p), device=dev)[:, :p]
    tht.copy_(theta)
    grad = torch.zeros(n, train.padded_ld(p), device=dev)[:, :p]
    bi = torch.zeros(n, b, dtype=torch.int32)
    for i, idx in enumerate(batches):
        bi[i, :idx.numel()] = (idx + i * s).to(torch.int32)
    bl = torch.tensor([v.numel() for v in batches], dtype=torch.int32, device=dev)
    rows = torch.arange(n, dtype=torch.int32, device=dev)
    loss = torch.empty(n, device=dev)
    args = (tht, x.reshape(n * s, -1).to(dev), y.to(torch.int32).to(dev), bi.to(dev), bl, rows, grad, loss)
    if cfg["model"] == "linear":
        torch.ops.niidmix.linear_nll_grad_rows(*args, Linear.K, Linear.C)
    else:
        torch.ops.niidmix.gnlenet_nll_grad_rows(*args, *GNNet.SHAPE)
    g = grad.cpu()
    for i, nd in enumerate(nodes):
        off = 0
        for q in nd["model"].parameters():
            q.grad = g[i, off:off + q.numel()].view_as(q).clone()
            off += q.numel()
    _reference_gradient(nodes, topo, params)
    oracle_mod.reference_loop_average(nodes, topo)
    return _flat(nodes), loss.cpu()


def _rounds_equal_their_parts(cfg, rounds, dev, oracle_mod, **kw):
    from niidmix import d_sgd, train
    params, nodes, topo, state = _setup(cfg, **kw)
    got = []
    for _ in range(rounds):
        state, losses, _, active = d_sgd.next_step(state, params, None)
        d_sgd.synchronize()
        assert active is nodes
        got.append((_flat(nodes), [losses[r] for r in range(cfg["n"])]))
    tr = d_sgd._trainers[id(nodes)]
    params2, twin, topo2, _ = _setup(cfg, **kw)                  # same seed: same models, same RNG
    for k in range(rounds):
        batches, _ = train.draw(twin, params2)
        want, loss = _parts_round(cfg, batches, topo2, twin, params2, dev, oracle_mod)
        assert torch.equal(_bits(got[k][0]), _bits(want)), f"round {k}"
        assert got[k][1] == loss.tolist(), f"round {k}"
    return tr, nodes, twin


@pytest.mark.parametrize("momentum", [0.0, MOM])
def test_linear_rounds_equal_their_parts(momentum, gpu, oracle_mod):
    """12 nodes in cliques of 4, 4 and 3 plus node 11 in none, connected, MH weights; two rounds
    (the non-first momentum step runs).  After each next_step the models equal, bit for bit, the
    gradient op on the same drawn indices, (b) on the CPU, then reference_loop_average.  Node 11
    is only mixed, never stepped."""
    tr, nodes, twin = _rounds_equal_their_parts(LIN, 2, gpu, oracle_mod, momentum=momentum)
    assert tr.grad_kind == "clique" and tr.gavg is None
    assert tr.segments[0].tolist() == [0, 4, 8, 11] and tr.segments[1].tolist() == [r for c in LIN["cliques"] for r in c]
    assert not twin[11]["optimizer"].state                          # the reference never stepped it
    if momentum:
        assert tr.mom_steps == 2
        assert not bool(tr.mbuf[11].any()) and bool(tr.mbuf[10].any())


def test_removed_clique_edges(gpu, oracle_mod):
    """remove-clique-edges with the intra-clique edge 0 - 2 missing: per-row lists."""
    tr, _, _ = _rounds_equal_their_parts(LIN, 1, gpu, oracle_mod, momentum=MOM, removed=True)
    assert tr.grad_kind == "clique-removed" and tr.gavg is not None
    assert tr.step_rows.tolist() == [r for c in LIN["cliques"] for r in c]


def test_unbiased_gradient(gpu, oracle_mod):
    """--unbiased-gradient with neighbourhoods of unequal lengths."""
    tr, _, _ = _rounds_equal_their_parts(LIN, 1, gpu, oracle_mod, momentum=MOM, avg="unbiased-gradient")
    assert tr.grad_kind == "unbiased" and tr.step_rows.tolist() == list(range(12))


def test_gn_lenet_round_equals_its_parts(gpu, oracle_mod):
    """--device-training-gn-lenet --clique-gradient, momentum 0.9: 4 nodes in two cliques, batch 2."""
    tr, _, _ = _rounds_equal_their_parts(GN, 1, gpu, oracle_mod, momentum=MOM)
    assert tr.kind == "gn-lenet" and tr.grad_kind == "clique"


def test_seven_rounds_against_the_cpu_path(gpu):
    """--clique-gradient: (a) flag off, (b) the same rounds in float64 torch with the cliques' mean
    gradient and a dense W^T theta mixing, (c) flag on; same seed, hence the same indices.
    max|theta_c - theta_b| <= 10 max|theta_a - theta_b| (tests/test_gpu_train.py's yardstick: the
    reference path's own fp32 drift, x10 for another summation order), and the mean loss falls."""
    from niidmix import d_sgd, train
    cfg, rounds = LIN, 7
    n, s = cfg["n"], cfg["s"]

    def run(flag):
        params, nodes, _, state = _setup(cfg, flag)
        losses = []
        for _ in range(rounds):
            state, ls, _, _ = d_sgd.next_step(state, params, None)
            d_sgd.synchronize()
            losses.append([ls[r] for r in range(n)])
        return _flat(nodes), losses

    th_a, loss_a = run(False)
    th_c, loss_c = run(True)

    params, nodes, topo, _ = _setup(cfg, True)
    x, y = _dataset(cfg)
    k, c = Linear.K, Linear.C
    tht = _flat(nodes).double()
    wt = topo["weights"].double().t()
    for _ in range(rounds):
        batches, _ = train.draw(nodes, params)
        g = torch.zeros_like(tht)
        for i, idx in enumerate(batches):
            w, b = tht[i, :c * k].view(c, k), tht[i, c * k:]
            _, g[i], _ = train.fp64_reference(w, b, x[idx + i * s], y[idx + i * s])
        for clique in topo["cliques"]:
            tht[clique] -= cfg["lr"] * g[clique].mean(0)
        tht = wt @ tht
    drift_a = float((th_a.double() - tht).abs().max())
    drift_c = float((th_c.double() - tht).abs().max())
    print(f"seven rounds, clique gradient: max|theta_a - theta_b| {drift_a:.3g}  "
          f"max|theta_c - theta_b| {drift_c:.3g}")
    assert drift_c <= 10 * drift_a
    mean = [sum(ls) / n for ls in loss_c]
    assert mean[-1] < mean[0]
    assert all(abs(c_ - a_) <= 1e-5 * abs(a_) for a_, c_ in zip(loss_a[0], loss_c[0]))
