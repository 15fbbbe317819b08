"""--device-training-large-batch on the GPU: niidmix::linear_nll_grad_rows_sliced against the float64
yardstick of tests/test_gpu_train.py (same bound), its layout and determinism contracts, the shape
both gradient ops take, and the plugin's rounds beyond batch-size * C = 32768 -- a 2-node ring bit
for bit against the same rounds assembled from the sliced op, the existing step and the existing
mixing (host sampling and --device-sampling-cached), and the centralised baseline of one node."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import test_gpu_sampling as tgsamp

pytestmark = pytest.mark.gpu

RTOL = 1e-5          # tests/test_gpu_train.py's: the project's fast-mode tolerance on the bound A
SENTINEL = 12345.678
SEED = tgsamp.SEED
LARGE = "device-training-large-batch"


# ------------------------------------------------------------------------------------------------
# 1. the op against float64
#   (K, C): layout.  'odd': ld = P + 3 (unaligned rows, scalar accesses); 'vec': ld = P rounded up to
#   4.  (6, 3) and (7, 10) take the scalar loads, (260, 17) two column chunks of float4 gathers and
#   two class blocks, (12, 8) the float4 staging of dz (C % 4 == 0).
SHAPES = {(6, 3): "vec", (7, 10): "odd", (260, 17): "vec", (12, 8): "vec"}
_cache = {}


def _case(k, c):
    """Inputs and float64 references of the two calls of a shape, computed once: a pool of 4 S
    samples, indices with repeats; call 0 has b_max = 3 S + 5 and lengths (1, S + 1, 3 S + 5), call
    1 b_max = 2 S and lengths (S - 1, S, 2 S + 7): the last is clamped to b_max."""
    if (k, c) in _cache:
        return _cache[(k, c)]
    from niidmix import ops, train
    s = ops.linear_sliced_slice(c)
    gen = torch.Generator().manual_seed(1000 * k + c)
    pool = 4 * s
    x = torch.rand(pool, k, generator=gen)
    y = torch.randint(0, c, (pool,), generator=gen)
    theta = torch.stack([torch.cat([(torch.rand(c, k, generator=gen) - 0.5).reshape(-1) * 2 / k ** 0.5,
                                    torch.rand(c, generator=gen) - 0.5]) for _ in range(3)])
    calls = []
    for b_max, lens in ((3 * s + 5, (1, s + 1, 3 * s + 5)), (2 * s, (s - 1, s, 2 * s + 7))):
        idx = torch.randint(0, pool, (3, b_max), generator=gen)
        l64, g64, bound = [], [], []
        for i in range(3):
            n = min(lens[i], b_max)
            w, b = theta[i, :c * k].view(c, k), theta[i, c * k:]
            ls, g, a = train.fp64_reference(w, b, x[idx[i, :n]], y[idx[i, :n]])
            l64.append(ls), g64.append(g), bound.append(a)
        calls.append(dict(b_max=b_max, lens=lens, idx=idx, l64=torch.stack(l64), g64=torch.stack(g64),
                          bound=torch.stack(bound)))
    out = dict(k=k, c=c, s=s, x=x, y=y, theta=theta, calls=calls)
    _cache[(k, c)] = out
    return out


def _launch(op, d, call, dev, layout, rows=(4, 0, 2), n_slab=6):
    """`op` on a call of a case: the three jobs are the listed rows `rows` (out of order) of an
    n_slab-row slab.  Returns (the grad slab with its padding columns, the losses)."""
    k, c = d["k"], d["c"]
    p = c * k + c
    ld = (p + 3) // 4 * 4 if layout == "vec" else p + 3
    th = torch.zeros(n_slab, ld, device=dev)
    for i, r in enumerate(rows):
        th[r, :p] = d["theta"][i].to(dev)
    grad = torch.full((n_slab, ld), SENTINEL, device=dev)
    loss = torch.zeros(3, device=dev)
    op(th[:, :p], d["x"].to(dev), d["y"].to(torch.int32).to(dev),
       call["idx"].to(torch.int32).to(dev).contiguous(),
       torch.tensor(call["lens"], dtype=torch.int32, device=dev),
       torch.tensor(rows, dtype=torch.int32, device=dev), grad[:, :p], loss, k, c)
    torch.cuda.synchronize()
    return grad.cpu(), loss.cpu()


def _check(grad, loss, d, call, rows, what):
    """The yardstick's bound on every listed row; the sentinel everywhere else."""
    p = d["c"] * d["k"] + d["c"]
    s = torch.tensor(SENTINEL)
    for r in range(grad.shape[0]):
        if r in rows:
            assert bool((grad[r, p:] == s).all()), f"{what}: row {r}: padding written"
        else:
            assert bool((grad[r] == s).all()), f"{what}: unlisted row {r} written"
    g = torch.stack([grad[r, :p] for r in rows])
    err = (g.double() - call["g64"]).abs()
    worst = float((err / call["bound"].clamp_min(1e-300)).max())
    dl = (loss.double() - call["l64"]).abs()
    print(f"{what}: worst |g - g64| / A {worst:.3g} (bound {RTOL}), worst loss error {float(dl.max()):.3g}")
    assert bool((err <= RTOL * call["bound"]).all()), f"{what}: {worst:.3g}"
    assert bool((dl <= RTOL * call["l64"].abs().clamp_min(1)).all()), what


@pytest.mark.parametrize("k,c", list(SHAPES))
def test_sliced_op_against_float64(k, c, gpu):
    """Every gradient element within 1e-5 A of float64, the loss within 1e-5 max(1, |loss64|), at
    lengths on both sides of one, two and three slices; rows not listed and grad's padding keep
    their sentinel; a batch_len above b_max is clamped."""
    from niidmix import ops  # noqa: F401  (registers the op)
    d = _case(k, c)
    rows = (4, 0, 2)
    for j, call in enumerate(d["calls"]):
        grad, loss = _launch(torch.ops.niidmix.linear_nll_grad_rows_sliced, d, call, gpu, SHAPES[(k, c)], rows)
        _check(grad, loss, d, call, rows, f"K {k} C {c} call {j}")


def test_sliced_op_gives_the_same_bits_twice(gpu):
    """Two launches on the same inputs (not a loop): equal bits, sentinel included."""
    from niidmix import ops  # noqa: F401
    for k, c in ((7, 10), (260, 17)):
        d = _case(k, c)
        a = _launch(torch.ops.niidmix.linear_nll_grad_rows_sliced, d, d["calls"][0], gpu, SHAPES[(k, c)])
        b = _launch(torch.ops.niidmix.linear_nll_grad_rows_sliced, d, d["calls"][0], gpu, SHAPES[(k, c)])
        assert torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)), (k, c)
        assert torch.equal(a[1].view(torch.int32), b[1].view(torch.int32)), (k, c)


def test_both_ops_meet_the_yardstick_where_both_take_the_shape(gpu):
    """C = 3, b_max = 2 S (b_max * C = 6144 <= MAX_BC): the sliced op and the existing op are both
    within the bound; equality between them is not required (another summation order)."""
    from niidmix import ops
    d = _case(6, 3)
    call = d["calls"][1]
    assert call["b_max"] == 2 * d["s"] and call["b_max"] * 3 <= ops.MAX_BC
    rows = (4, 0, 2)
    for name in ("linear_nll_grad_rows_sliced", "linear_nll_grad_rows"):
        grad, loss = _launch(getattr(torch.ops.niidmix, name), d, call, gpu, "vec", rows)
        _check(grad, loss, d, call, rows, name)


# ------------------------------------------------------------------------------------------------
# 2. the plugin's rounds
class Net(torch.nn.Module):
    def __init__(self, k, c):
        super().__init__()
        self.k = k
        self.fc = torch.nn.Linear(k, c)

    def forward(self, x, params):
        return F.log_softmax(self.fc(x.view(-1, self.k)), dim=1)


LR = 0.1
_data = {}


def _dataset(k, c, total):
    if (k, c, total) not in _data:
        g = torch.Generator().manual_seed(77 + total)
        x = torch.randn(total, k, generator=g)
        _data[(k, c, total)] = (x, torch.randint(0, c, (total,), generator=g))
    return _data[(k, c, total)]


def _setup(k, c, sizes, batch, topo_name, topo, momentum=0.0, flags=(LARGE,)):
    """Nodes with train-sets of `sizes` samples and the plugin's state (d_sgd.init)."""
    from niidmix import d_sgd
    torch.manual_seed(2030)
    params = {"meta": {"log": "WARNING", "seed": SEED}, "nodes": {"nb-nodes": len(sizes)},
              "topology": {"name": topo_name, "remove-clique-edges": 0},
              "logger": {"accuracy-logging-interval": 0, "accuracy-logging-interval-steps": 0,
                         "log-consensus-distance": False},
              "algorithm": {"learning-rate": LR, "learning-momentum": momentum, "batch-size": batch,
                            "initial-averaging": False, "clique-gradient": False,
                            "unbiased-gradient": False, "deferred-writeback": False,
                            "mixing-mode": "exact", "device-training": True, **{f: True for f in flags}}}
    x, y = _dataset(k, c, sum(sizes))
    start = np.cumsum([0] + list(sizes))
    nodes = []
    for r in range(len(sizes)):
        mdl = Net(k, c)
        nodes.append({"rank": r, "epoch": 0, "model": mdl, "optimizer": d_sgd.optimizer(mdl, params),
                      "train-set": [(x[j], int(y[j])) for j in range(start[r], start[r + 1])]})
    state, _, _ = d_sgd.init(nodes, topo, params)
    return params, nodes, state, start


def _flat(nodes):
    return torch.stack([torch.cat([q.detach().reshape(-1) for q in nd["model"].parameters()])
                        for nd in nodes]).clone()


RING2 = {"edges": {0: [1], 1: [0]}, "weights": torch.full((2, 2), 0.5)}
SIZES2 = (12000, 11000)


@pytest.mark.parametrize("sampling", [False, True], ids=["host-sampling", "device-sampling-cached"])
@pytest.mark.parametrize("momentum", [0.0, 0.9])
def test_two_rounds_equal_their_parts(momentum, sampling, gpu):
    """A 2-node ring of Net(6, 3), batch MAX_BC // 3 + 1, train-sets of 12 000 and 11 000 samples:
    after each of two next_step calls the parameters and losses equal, bit for bit, the round
    assembled from the sliced op, the existing step op and the existing mixing on the same indices
    -- those a twin's loaders draw from the same RNG stream, or, under --device-sampling
    --device-sampling-cached, those of niidmix.sampling's restatement (the second round is the
    epoch's short tail: 1077 and 77 samples)."""
    from niidmix import d_sgd, ops, train
    from niidmix.sampling import SamplerState
    from niidmix.topology import to_csr
    k, c, n = 6, 3, 2
    batch = ops.MAX_BC // c + 1
    assert batch * c > ops.MAX_BC
    flags = (LARGE, "device-sampling", "device-sampling-cached") if sampling else (LARGE,)
    params, nodes, state, start = _setup(k, c, SIZES2, batch, "ring", RING2, momentum, flags)
    theta0 = _flat(nodes)
    if sampling:
        st = SamplerState(range(n), SIZES2, batch)
    else:
        params2, twin, _, _ = _setup(k, c, SIZES2, batch, "ring", RING2, momentum, flags)   # same seed: same RNG
        assert torch.equal(_flat(twin), theta0)
        rng = torch.get_rng_state()

    p = c * k + c
    x, y = _dataset(k, c, sum(SIZES2))
    ld = train.padded_ld(p)
    th, th2, grad, buf = (torch.zeros(n, ld, device=gpu)[:, :p] for _ in range(4))
    th.copy_(theta0)
    data, labels = x.to(gpu), y.to(torch.int32).to(gpu)
    rows = torch.arange(n, dtype=torch.int32, device=gpu)
    mixer = ops.Mixer(csr=to_csr(RING2), device=gpu)
    want_lens = [(batch, batch), (SIZES2[0] - batch, SIZES2[1] - batch)]
    for rnd in range(2):
        if not sampling:
            torch.set_rng_state(rng)             # the run under test draws from the stream the twin drew from
            state, losses, done, _ = d_sgd.next_step(state, params, None)
            after = torch.get_rng_state()
            torch.set_rng_state(rng)
            batches, want_done = train.draw(twin, params2)
            rng = torch.get_rng_state()
            assert torch.equal(rng, after)
        else:
            state, losses, done, _ = d_sgd.next_step(state, params, None)
            epoch, cursor, want_done = st.advance(range(n))
            batches = [torch.from_numpy(tgsamp._perm(r, int(epoch[r]), SIZES2[r])[cursor[r]:cursor[r] + batch].copy())
                       for r in range(n)]
        d_sgd.synchronize()
        assert done == want_done and tuple(b.numel() for b in batches) == want_lens[rnd]
        tr = d_sgd._trainers[id(nodes)]
        assert tr.large and tr.family.sliced(tr.b_max, tr.sizes, tr.large) and tr.last_calls == 1
        bi = torch.zeros(n, batch, dtype=torch.int32)
        for i, idx in enumerate(batches):
            bi[i, :idx.numel()] = (idx + int(start[i])).to(torch.int32)
        bl = torch.tensor([b.numel() for b in batches], dtype=torch.int32)
        got_bi = tr.layout.view(tr.idx_dev, "indices").cpu()
        for i in range(n):                       # the index block the gradient op read
            assert torch.equal(got_bi[i, :int(bl[i])], bi[i, :int(bl[i])]), (rnd, i)
        loss = torch.empty(n, device=gpu)
        torch.ops.niidmix.linear_nll_grad_rows_sliced(th, data, labels, bi.to(gpu), bl.to(gpu), rows,
                                                      grad, loss, k, c)
        if momentum:
            torch.ops.niidmix.sgd_momentum_step_rows(th, grad, buf, rows, -LR, momentum, rnd == 0)
        else:
            torch.ops.niidmix.sgd_step_rows(th, grad, rows, -LR)
        mixer(th, out=th2, mode="exact")
        th, th2 = th2, th
        assert torch.equal(_flat(nodes).view(torch.int32), th.cpu().view(torch.int32)), f"round {rnd}"
        assert [losses[r] for r in range(n)] == loss.cpu().tolist(), f"round {rnd}"
    assert not torch.equal(theta0, _flat(nodes))
    assert done == {0: True, 1: True}            # both epochs ended with the second round's tail


ONE = {"edges": {0: []}, "weights": torch.tensor([[1.0]])}


def test_one_node_is_the_centralised_baseline(gpu):
    """One node, 'fully-connected', batch 12 800 on 13 000 samples, K = 6, C = 10, three rounds:
    12 800 samples, the tail of 200 (which ends the epoch), 12 800 again.  Each round's loss is
    within 1e-5 max(1, |loss64|) of float64 at the parameters the round started from, and its
    parameters within the gradient's bound propagated by one step: |theta' - (theta - lr g64)| <=
    lr 1e-5 A + 2^-23 (|theta| + lr |g64|) -- the second term covers the fp32 step's own roundings
    (lr g and the difference, half an ulp each, and lr's representation).  Mixing one node is
    theta' = 1.0 theta, exact."""
    from niidmix import d_sgd, train
    k, c, batch, size = 6, 10, 12800, 13000
    params, nodes, state, _ = _setup(k, c, (size,), batch, "fully-connected", ONE)
    params2, twin, _, _ = _setup(k, c, (size,), batch, "fully-connected", ONE)
    rng = torch.get_rng_state()
    x, y = _dataset(k, c, size)
    dones, lens = [], []
    for rnd in range(3):
        theta = _flat(nodes)[0]
        torch.set_rng_state(rng)
        state, losses, done, active = d_sgd.next_step(state, params, None)
        d_sgd.synchronize()
        torch.set_rng_state(rng)
        (idx,), _ = train.draw(twin, params2)
        rng = torch.get_rng_state()
        dones.append(done[0]), lens.append(idx.numel())
        w, b = theta[:c * k].view(c, k), theta[c * k:]
        l64, g64, a = train.fp64_reference(w, b, x[idx], y[idx])
        want = theta.double() - LR * g64
        err = (_flat(nodes)[0].double() - want).abs()
        bound = LR * RTOL * a + 2.0 ** -23 * (theta.double().abs() + LR * g64.abs())
        print(f"round {rnd}: {idx.numel()} samples, loss {losses[0]:.6f} (float64 {float(l64):.6f}), "
              f"worst parameter error / bound {float((err / bound).max()):.3g}")
        assert abs(losses[0] - float(l64)) <= RTOL * max(1.0, abs(float(l64))), f"round {rnd}"
        assert bool((err <= bound).all()), f"round {rnd}"
        assert active is nodes and sorted(losses) == [0]
    assert lens == [batch, size - batch, batch]
    assert dones == [False, True, False] and nodes[0]["epoch"] == 1
    tr = d_sgd._trainers[id(nodes)]
    assert tr.n == 1 and tr.large and tr.family.sliced(tr.b_max, tr.sizes, True)


def test_unflagged_run_keeps_the_existing_refusal(gpu):
    from niidmix import ops
    with pytest.raises(ValueError, match=rf"--device-training: C = 10, batch-size \* C = 128000 exceed the "
                                         rf"kernel's limits \(C <= 1024, batch-size \* C <= {ops.MAX_BC}\)"):
        _setup(6, 10, (13000,), 12800, "fully-connected", ONE, flags=())
