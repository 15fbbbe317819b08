"""--device-training-gn-lenet on the GPU: niidmix::gnlenet_nll_grad_rows against float64 autograd
over the functional forward (niidmix.train.fp64_reference_gn_lenet, which
tests/test_train_gnlenet_host.py pins to the reference's own gradients), the kernel's contracts,
and the plugin's rounds with the flag on.

Accuracy: g64 is the yardstick, g32 the same autograd in torch fp32 on the CPU.  Per tensor t,
r32_t = max|g32_t - g64_t| / max|g64_t|, and e32 = max_t r32_t over the 14 tensors of the case's
rows (pooled: one small tensor's maximum is too noisy a yardstick).  The kernel must satisfy
max|g_t - g64_t| / max|g64_t| <= 4 e32 for every t and |loss - loss64| <= 4 e32 max(1, |loss64|): its
error is of torch fp32's kind under another summation order (the factor 4 is the forward's in
tests/test_gpu_eval_gnlenet.py), an indexing or routing bug is ~1e5 e32.

A pool argmax or a ReLU sign that flips between precisions changes the gradient discontinuously,
so every seeded case is well separated in float64: with e_act = max|fp32 - float64| over the
case's intermediate maps, every pool window's top-two gap and every pre-ReLU magnitude exceed
16 e_act (the seeds were chosen on the CPU so that this holds without exception).
"""
import math

import pytest
import torch
import torch.nn.functional as F

import test_eval_gnlenet_host as th

pytestmark = pytest.mark.gpu

FACTOR = 4
# (Cin, H, W, C, rows, b_max, lengths, seed): every pooled map at its minimum (7 / 3 / 1);
# non-square and odd; the reference's two shapes; one class; a large shape
CASES = [(1, 15, 15, 3, 3, 4, (4, 1, 3), 2030),
         (3, 17, 15, 10, 2, 3, (3, 2), 2091),
         (1, 28, 28, 10, 2, 3, (3, 3), 2452),
         (3, 32, 32, 10, 2, 3, (2, 3), 7333),
         (1, 28, 28, 1, 1, 2, (2,), 2134),
         (2, 40, 36, 4, 2, 2, (2, 1), 3505)]
_ids = ["x".join(map(str, c[:4])) for c in CASES]
_cache = {}


def stages(ts, x):
    """The maps the discontinuities sit on: ([maps that are max-pooled], [maps that are ReLU'd])."""
    c1 = F.conv2d(x, ts[0], ts[1], padding=2)
    n1 = F.group_norm(F.max_pool2d(c1, 3, 2), 2, ts[2], ts[3], 1e-5)
    n2 = F.group_norm(F.conv2d(F.relu(n1), ts[4], ts[5], padding=2), 2, ts[6], ts[7], 1e-5)
    p2 = F.max_pool2d(n2, 3, 2)
    n3 = F.group_norm(F.conv2d(F.relu(p2), ts[8], ts[9], padding=2), 2, ts[10], ts[11], 1e-5)
    p3 = F.max_pool2d(n3, 3, 2)
    return [c1, n2, n3], [n1, p2, p3]


def separation(theta_row, x):
    """(e_act, smallest pool top-two gap, smallest pre-ReLU magnitude) of one row on its batch."""
    from niidmix import train
    cin, hw = int(x.shape[1]), (int(x.shape[2]), int(x.shape[3]))
    with torch.no_grad():
        p64, r64 = stages(train.split_gn_lenet(theta_row.double(), cin, hw), x.double())
        p32, r32 = stages(train.split_gn_lenet(theta_row, cin, hw), x)
    e_act = max(float((a.double() - b).abs().max()) for a, b in zip(p32 + r32, p64 + r64))
    gap = math.inf
    for m in p64:
        b, c, h, w = m.shape
        win = F.unfold(m.reshape(b * c, 1, h, w), 3, stride=2)          # [b c, 9, windows]
        top = win.topk(2, dim=1).values
        gap = min(gap, float((top[:, 0] - top[:, 1]).min()))
    mag = min(float(m.abs().min()) for m in r64)
    return e_act, gap, mag


def make_case(cin, h, w, c, n_rows, b_max, lens, seed, background=False):
    """Inputs of a case: n_rows perturbed models, n_rows * b_max samples, per row a batch of
    distinct indices into all of them."""
    torch.manual_seed(seed)
    gen = torch.Generator().manual_seed(seed)
    theta = torch.stack([torch.cat([q.detach().reshape(-1) for q in
                                    th.perturb(th.GNLeNet(cin, c, (h, w)), gen).parameters()])
                         for _ in range(n_rows)])
    s = n_rows * b_max
    x = torch.randn(s, cin, h, w, generator=gen)
    if background:                         # MNIST-like: a lit centre on an all-zero background
        mask = torch.zeros(h, w)
        mask[h // 3:h - h // 3, w // 3:w - w // 3] = 1.0
        x = x * mask
    y = torch.randint(0, c, (s,), generator=gen)
    idx = torch.stack([torch.randperm(s, generator=gen)[:b_max] for _ in range(n_rows)])
    return dict(shape=(cin, h, w, c), theta=theta, x=x, y=y, idx=idx, lens=list(lens), p=theta.shape[1],
                n_rows=n_rows, b_max=b_max)


def rel(err, top):
    """err relative to a tensor's largest float64 element; a tensor that is exactly zero in float64
    (every gradient of a one-class model: softmax is 1) admits no error at all."""
    return err / top if top > 0 else (0.0 if err == 0 else math.inf)


def add_references(d):
    """Per row (loss64, g64), (loss32, g32), computed once; e32 pooled over tensors and rows."""
    from niidmix import train
    cin, h, w, c = d["shape"]
    off = train.gn_lenet_offsets(cin, c, th.sizes(cin, h, w, c)[0])
    d["off"] = off
    d["ref"], e32 = [], 0.0
    for r in range(d["n_rows"]):
        ix = d["idx"][r, :d["lens"][r]]
        l64, g64 = train.fp64_reference_gn_lenet(d["theta"][r], d["x"][ix], d["y"][ix])
        l32, g32 = train.reference_gn_lenet(d["theta"][r], d["x"][ix], d["y"][ix], torch.float32)
        d["ref"].append((l64, g64, l32, g32))
        for t in range(14):
            a, b = g32[off[t]:off[t + 1]].double(), g64[off[t]:off[t + 1]]
            e32 = max(e32, rel(float((a - b).abs().max()), float(b.abs().max())))
    d["e32"] = e32
    return d


def _case(i):
    if i not in _cache:
        _cache[i] = add_references(make_case(*CASES[i]))
    return _cache[i]


def _launch(d, dev, layout="vec", order=None, theta=None, idx=None, lens=None):
    """The op on rows `order` (entries of the case, default all) of a slab with one spare row, the
    case's row r at slab row perm[r] (a non-identity permutation).  Returns (grad slab, loss,
    slab rows, theta before, theta after); unlisted rows and pad columns of grad hold -7."""
    cin, h, w, c = d["shape"]
    p, n, b_max = d["p"], d["n_rows"], d["b_max"]
    ld = (p + 3) // 4 * 4 + 4 if layout == "vec" else p + 1
    perm = [(r + 1) % (n + 1) for r in range(n)]
    slab = torch.zeros(n + 1, ld, device=dev)
    src = d["theta"] if theta is None else theta
    for r in range(n):
        slab[perm[r], :p] = src[r].to(dev)
    before = slab.clone()
    grad = torch.full((n + 1, ld), -7.0, device=dev)
    order = list(range(n)) if order is None else order
    lens = d["lens"] if lens is None else lens
    idx = d["idx"] if idx is None else idx
    bi = idx[order].to(torch.int32).contiguous().to(dev)
    bl = torch.tensor([lens[r] for r in order], dtype=torch.int32, device=dev)
    rows = torch.tensor([perm[r] for r in order], dtype=torch.int32, device=dev)
    loss = torch.full((len(order),), -7.0, device=dev)
    torch.ops.niidmix.gnlenet_nll_grad_rows(slab[:, :p], d["x"].reshape(n * b_max, -1).to(dev),
                                            d["y"].to(torch.int32).to(dev), bi, bl, rows, grad[:, :p],
                                            loss, cin, h, w, c)
    torch.cuda.synchronize()
    return grad.cpu(), loss.cpu(), perm, before.cpu(), slab.cpu()


def _bits(t):
    return t.contiguous().view(torch.int32)


def _check_accuracy(d, grad, loss, perm, what):
    """Every listed row's tensors and loss within FACTOR e32 of float64; prints the ratios."""
    off, e32, p = d["off"], d["e32"], d["p"]
    worst, worst_l = 0.0, 0.0
    for r in range(d["n_rows"]):
        l64, g64 = d["ref"][r][:2]
        g = grad[perm[r], :p].double()
        for t in range(14):
            err = float((g[off[t]:off[t + 1]] - g64[off[t]:off[t + 1]]).abs().max())
            worst = max(worst, rel(err, float(g64[off[t]:off[t + 1]].abs().max())))
        worst_l = max(worst_l, abs(float(loss[r]) - float(l64)) / max(1.0, abs(float(l64))))
    ratio = lambda v: v / e32 if e32 else (0.0 if v == 0 else math.inf)  # noqa: E731
    print(f"{what}: e32 {e32:.3g}  gradient ratio {ratio(worst):.3g}  loss ratio {ratio(worst_l):.3g}")
    assert worst <= FACTOR * e32, f"gradient off by {ratio(worst):.3g} e32"
    assert worst_l <= FACTOR * e32, f"loss off by {ratio(worst_l):.3g} e32"


def _check_sentinels(d, grad, perm, before, after):
    p, n = d["p"], d["n_rows"]
    assert torch.equal(_bits(before), _bits(after)), "theta was written"
    spare = [r for r in range(n + 1) if r not in perm]
    assert bool((grad[spare] == -7.0).all()), "an unlisted row of grad was written"
    assert bool((grad[:, p:] == -7.0).all()), "a pad column of grad was written"


@pytest.mark.parametrize("layout", ["vec", "odd"])
@pytest.mark.parametrize("i", range(len(CASES)), ids=_ids)
def test_kernel_against_float64(i, layout, gpu):
    from niidmix import ops  # noqa: F401  (registers the op)
    d = _case(i)
    for r in range(d["n_rows"]):
        ix = d["idx"][r, :d["lens"][r]]
        e_act, gap, mag = separation(d["theta"][r], d["x"][ix])
        assert gap > 16 * e_act and mag > 16 * e_act, \
            f"reseed the case: e_act {e_act:.3g}, pool gap {gap:.3g}, pre-ReLU magnitude {mag:.3g}"
    grad, loss, perm, before, after = _launch(d, gpu, layout=layout)
    _check_sentinels(d, grad, perm, before, after)
    _check_accuracy(d, grad, loss, perm, f"{_ids[i]} {layout}")


def test_pool_ties_take_the_first_maximum(gpu):
    """An all-zero background: conv1 is exactly its bias there, in fp32 and float64 alike, so the
    first pool's windows tie and the first-maximum rule decides where the gradient goes."""
    from niidmix import ops  # noqa: F401
    d = add_references(make_case(1, 28, 28, 10, 2, 3, (3, 2), 2100, background=True))
    grad, loss, perm, before, after = _launch(d, gpu)
    _check_sentinels(d, grad, perm, before, after)
    _check_accuracy(d, grad, loss, perm, "pool ties")


@pytest.mark.parametrize("i", [0, 3], ids=[_ids[0], _ids[3]])
def test_determinism_and_independence(i, gpu):
    """Two calls give equal bits; a row alone = the row among others = the row list split over two
    calls, bitwise; the leading dimension does not enter."""
    from niidmix import ops  # noqa: F401
    d = _case(i)
    p, n = d["p"], d["n_rows"]
    a = _launch(d, gpu)
    b = _launch(d, gpu)
    assert torch.equal(_bits(a[0]), _bits(b[0])) and torch.equal(_bits(a[1]), _bits(b[1]))
    perm = a[2]
    for r in range(n):
        g, ls = _launch(d, gpu, order=[r])[:2]
        assert torch.equal(_bits(g[perm[r], :p]), _bits(a[0][perm[r], :p])), r
        assert torch.equal(_bits(ls[0]), _bits(a[1][r])), r
    lo, hi = _launch(d, gpu, order=[n - 1]), _launch(d, gpu, order=list(range(n - 1))[::-1])
    assert torch.equal(_bits(lo[0][perm[n - 1], :p]), _bits(a[0][perm[n - 1], :p]))
    for k, r in enumerate(list(range(n - 1))[::-1]):
        assert torch.equal(_bits(hi[0][perm[r], :p]), _bits(a[0][perm[r], :p]))
        assert torch.equal(_bits(hi[1][k]), _bits(a[1][r]))
    c = _launch(d, gpu, layout="odd")
    for r in range(n):
        assert torch.equal(_bits(c[0][perm[r], :p]), _bits(a[0][perm[r], :p]))
    assert torch.equal(_bits(c[1]), _bits(a[1]))


def test_a_batch_with_a_repeated_index(gpu):
    from niidmix import ops, train  # noqa: F401
    d = dict(_case(1))
    idx = d["idx"].clone()
    idx[0, 2] = idx[0, 0]
    d["idx"] = idx
    d = add_references(d)
    grad, loss, perm, before, after = _launch(d, gpu)
    _check_accuracy(d, grad, loss, perm, "repeated index")


def test_nan_stays_in_its_row(gpu):
    """A NaN in row 1's conv2.w: only that row's grad and loss are non-finite, row 0's bits are
    those of the clean call."""
    from niidmix import ops, train  # noqa: F401
    d = _case(2)
    p = d["p"]
    clean = _launch(d, gpu)
    theta = d["theta"].clone()
    theta[1, d["off"][4] + 12345] = float("nan")
    grad, loss, perm, _, _ = _launch(d, gpu, theta=theta)
    assert math.isnan(float(loss[1])) and not bool(torch.isfinite(grad[perm[1], :p]).all())
    assert torch.equal(_bits(grad[perm[0], :p]), _bits(clean[0][perm[0], :p]))
    assert torch.equal(_bits(loss[0]), _bits(clean[1][0]))


@pytest.mark.parametrize("name", ["gn_lenet_mnist", "gn_lenet_cifar"])
def test_fixtures_through_the_op(name, gpu):
    """The reference's own model, samples and fp32 gradient: per tensor within 4 e32 plus the
    fixture's own distance from float64."""
    from niidmix import ops, train  # noqa: F401
    f, g = th.load_fixture(name), th.load_fixture(name + "_grad")
    cin, h, w, c = (int(v) for v in f["shape"])
    theta, x, y = torch.from_numpy(f["theta"]), torch.from_numpy(f["x"]), torch.from_numpy(f["y"])
    ref, ref_loss = torch.from_numpy(g["grad"]).double(), float(g["loss"])
    l64, g64 = train.fp64_reference_gn_lenet(theta, x, y)
    g32 = train.reference_gn_lenet(theta, x, y, torch.float32)[1].double()
    off = train.gn_lenet_offsets(cin, c, th.sizes(cin, h, w, c)[0])
    seg = [slice(off[t], off[t + 1]) for t in range(14)]
    e32 = max(float((g32[s] - g64[s]).abs().max()) / float(g64[s].abs().max()) for s in seg)
    dev = gpu
    grad = torch.zeros(1, theta.numel(), device=dev)
    loss = torch.zeros(1, device=dev)
    torch.ops.niidmix.gnlenet_nll_grad_rows(
        theta.reshape(1, -1).to(dev), x.reshape(4, -1).to(dev), y.to(torch.int32).to(dev),
        torch.arange(4, dtype=torch.int32, device=dev).reshape(1, 4),
        torch.tensor([4], dtype=torch.int32, device=dev), torch.zeros(1, dtype=torch.int32, device=dev),
        grad, loss, cin, h, w, c)
    got = grad[0].cpu().double()
    worst = 0.0
    for s in seg:
        top = float(g64[s].abs().max())
        r = float((ref[s] - g64[s]).abs().max()) / top
        err = float((got[s] - ref[s]).abs().max()) / top
        worst = max(worst, err / (FACTOR * e32 + r))
        assert err <= FACTOR * e32 + r, (err, e32, r)
    rl = abs(ref_loss - float(l64))
    print(f"{name}: e32 {e32:.3g}  worst (error / bound) {worst:.3g}")
    assert abs(float(loss[0]) - ref_loss) <= FACTOR * e32 * max(1.0, abs(float(l64))) + rl


def test_op_refuses_bad_arguments(gpu):
    from niidmix import ops  # noqa: F401
    d = _case(0)
    cin, h, w, c = d["shape"]
    p, dev = d["p"], gpu
    theta = d["theta"][:1].to(dev)
    x, y = d["x"].reshape(d["x"].shape[0], -1).to(dev), d["y"].to(torch.int32).to(dev)
    bi = d["idx"][:1].to(torch.int32).to(dev)
    bl = torch.tensor([2], dtype=torch.int32, device=dev)
    rows = torch.zeros(1, dtype=torch.int32, device=dev)
    grad, loss = torch.zeros(1, p, device=dev), torch.zeros(1, device=dev)
    op = torch.ops.niidmix.gnlenet_nll_grad_rows
    op(theta, x, y, bi, bl, rows, grad, loss, cin, h, w, c)                      # the good call
    with pytest.raises(RuntimeError):
        op(theta.cpu(), x, y, bi, bl, rows, grad, loss, cin, h, w, c)
    with pytest.raises(RuntimeError):
        op(theta.double(), x, y, bi, bl, rows, grad, loss, cin, h, w, c)
    with pytest.raises(RuntimeError):
        op(theta, x, y, bi.long(), bl, rows, grad, loss, cin, h, w, c)
    with pytest.raises(RuntimeError):
        op(theta, x, y, bi, bl, rows, theta, loss, cin, h, w, c)                 # grad aliases theta
    with pytest.raises(RuntimeError):
        op(theta, x, y, bi, bl, rows, grad[:, :p - 1], loss, cin, h, w, c)
    with pytest.raises(RuntimeError):
        op(theta, x, y, bi, bl, rows, grad, loss, cin, h, 14, c)


# ------------------------------------------------------------------------------------------------
# the plugin's round: a 4-node ring of (1, 15, 15, 3) models, batch 4
N, B, S, LR = 4, 4, 12, 0.05
SHAPE = (1, 15, 15, 3)


class Net(th.GNLeNet):
    def __init__(self, groups=2):
        super().__init__(SHAPE[0], SHAPE[3], SHAPE[1:3], groups)


class FourGroups(Net):
    def __init__(self):
        super().__init__(groups=4)


def _ring():
    w = torch.zeros(N, N)
    for i in range(N):
        for j in (i - 1, i, i + 1):
            w[i, j % N] = 1.0 / 3.0
    return {"edges": {i: [(i - 1) % N, (i + 1) % N] for i in range(N)}, "weights": w}


_data = {}


def _dataset():
    if not _data:
        g = torch.Generator().manual_seed(314)
        _data.update(x=torch.randn(N * S, *SHAPE[:3], generator=g),
                     y=torch.randint(0, SHAPE[3], (N * S,), generator=g))
    return _data["x"], _data["y"]


def _setup(flag, momentum=0.0, model=Net, evaluation=False):
    """flag: None (CPU training), "gn" (--device-training-gn-lenet)."""
    from niidmix import d_sgd
    torch.manual_seed(2025)
    params = {"meta": {"log": "WARNING", "seed": 2025}, "nodes": {"nb-nodes": N},
              "topology": {"name": "ring", "remove-clique-edges": 0},
              "logger": {"accuracy-logging-interval": 0, "accuracy-logging-interval-steps": 0,
                         "log-consensus-distance": False},
              "algorithm": {"learning-rate": LR, "learning-momentum": momentum, "batch-size": B,
                            "initial-averaging": False, "clique-gradient": False,
                            "unbiased-gradient": False, "deferred-writeback": False,
                            "mixing-mode": "exact"}}
    if flag == "gn":
        params["algorithm"]["device-training"] = True
        params["algorithm"]["device-training-gn-lenet"] = True
    if evaluation:
        params["algorithm"]["device-evaluation"] = True
    x, y = _dataset()
    gen = torch.Generator().manual_seed(2026)
    nodes = []
    for r in range(N):
        mdl = th.perturb(model(), gen)
        ts = [(x[r * S + j], int(y[r * S + j])) for j in range(S)]
        nodes.append({"rank": r, "epoch": 0, "train-set": ts, "model": mdl,
                      "optimizer": d_sgd.optimizer(mdl, params)})
    topo = _ring()
    state, _, _ = d_sgd.init(nodes, topo, params)
    return params, nodes, topo, state


def _flat(nodes):
    return torch.stack([torch.cat([q.detach().reshape(-1) for q in nd["model"].parameters()])
                        for nd in nodes]).clone()


def _parts_round(theta, batches, topo, nodes, momentum, dev, oracle_mod):
    """mix(step(theta, g_kernel)): the op on the same indices, the existing step op, the oracle's
    reference loop for the mixing."""
    from niidmix import model as nm, train
    x, y = _dataset()
    p = theta.shape[1]
    tht = torch.zeros(N, train.padded_ld(p), device=dev)[:, :p]
    tht.copy_(theta)
    grad = torch.zeros(N, train.padded_ld(p), device=dev)[:, :p]
    bi = torch.zeros(N, B, dtype=torch.int32)
    for i, idx in enumerate(batches):
        bi[i, :idx.numel()] = (idx + i * S).to(torch.int32)
    bl = torch.tensor([b.numel() for b in batches], dtype=torch.int32, device=dev)
    rows = torch.arange(N, dtype=torch.int32, device=dev)
    loss = torch.empty(N, device=dev)
    torch.ops.niidmix.gnlenet_nll_grad_rows(tht, x.reshape(N * S, -1).to(dev), y.to(torch.int32).to(dev),
                                            bi.to(dev), bl, rows, grad, loss, *SHAPE)
    if momentum:
        buf = torch.zeros(N, train.padded_ld(p), device=dev)[:, :p]
        torch.ops.niidmix.sgd_momentum_step_rows(tht, grad, buf, rows, -LR, momentum, True)
    else:
        torch.ops.niidmix.sgd_step_rows(tht, grad, rows, -LR)
    stepped = tht.cpu()
    for i, nd in enumerate(nodes):
        nm.unflatten_into(nd["model"], stepped[i])
    oracle_mod.reference_loop_average(nodes, topo)
    return _flat(nodes), loss.cpu()


@pytest.mark.parametrize("momentum", [0.0, 0.9])
def test_one_round_equals_its_parts(momentum, gpu, oracle_mod):
    """After one next_step under the flag the models equal, bit for bit, mix(step(theta, g)) with g
    from a direct call of the op on the same indices."""
    from niidmix import d_sgd, train
    params, nodes, topo, state = _setup("gn", momentum)
    state, losses, _, active = d_sgd.next_step(state, params, None)
    d_sgd.synchronize()
    got = _flat(nodes)
    assert active is nodes and sorted(losses) == list(range(N))
    tr = d_sgd._trainers[id(nodes)]
    assert tr.kind == "gn-lenet" and tr.sizes == SHAPE and tr.last_calls == 1

    params2, twin, topo2, _ = _setup("gn", momentum)               # same seed: same models, same RNG
    theta0 = _flat(twin)
    batches, _ = train.draw(twin, params2)
    want, loss = _parts_round(theta0, batches, topo2, twin, momentum, gpu, oracle_mod)
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    assert [losses[r] for r in range(N)] == loss.tolist()

    # the row list cut by a scratch budget of two rows: two calls, the same bits
    params3, third, _, state3 = _setup("gn", momentum)
    tr3 = d_sgd._trainer(third, state3["topology"], params3)
    tr3.scratch_budget = tr3._gn_need(2)
    d_sgd.next_step(state3, params3, None)
    d_sgd.synchronize()
    assert tr3.last_calls == 2
    assert torch.equal(_flat(third).view(torch.int32), got.view(torch.int32))


def test_seven_rounds_against_the_cpu_path(gpu):
    """(a) flag off, (b) the same rounds restated in float64, (c) flag on; same seed, hence the
    same samples.  max|theta_c - theta_b| <= 10 max|theta_a - theta_b| (tests/test_gpu_train.py's
    rule: the reference's own fp32 drift, x10 for another summation order)."""
    from niidmix import d_sgd, train
    rounds = 7

    def run(flag):
        params, nodes, _, state = _setup(flag)
        losses, dones = [], []
        for _ in range(rounds):
            state, ls, done, _ = d_sgd.next_step(state, params, None)
            d_sgd.synchronize()
            losses.append([ls[r] for r in range(N)])
            dones.append(done)
        return _flat(nodes), losses, dones

    th_a, loss_a, done_a = run(None)
    th_c, loss_c, done_c = run("gn")

    params, nodes, topo, _ = _setup("gn")
    x, y = _dataset()
    tht = _flat(nodes).double()
    wt = topo["weights"].double().t()
    for _ in range(rounds):
        batches, _ = train.draw(nodes, params)
        for i, idx in enumerate(batches):
            _, g = train.fp64_reference_gn_lenet(tht[i], x[idx + i * S], y[idx + i * S])
            tht[i] -= LR * g
        tht = wt @ tht
    drift_a = float((th_a.double() - tht).abs().max())
    drift_c = float((th_c.double() - tht).abs().max())
    print(f"seven rounds: max|theta_a - theta_b| {drift_a:.3g}  max|theta_c - theta_b| {drift_c:.3g}")
    assert drift_c <= 10 * drift_a
    assert done_a == done_c and any(any(d.values()) for d in done_c)      # identical samples drawn


def test_probe_refuses_another_group_count(gpu):
    """GroupNorm(4, .) has GN-LeNet's parameter shapes: only the forward / backward probe can tell."""
    from niidmix import d_sgd
    params, nodes, topo, state = _setup("gn", model=FourGroups)
    with pytest.raises(ValueError, match="device-training-gn-lenet"):
        d_sgd.next_step(state, params, None)


def test_live_cpu_momentum_buffers_are_refused(gpu):
    """The flag switched on after a CPU momentum step: the trainer refuses to take the buffers
    over, with a ValueError naming the flag in use."""
    from niidmix import d_sgd
    params, nodes, topo, state = _setup(None, momentum=0.9)
    x, y = _dataset()
    for nd in nodes:                                               # a CPU optimizer step: buffers exist
        F.nll_loss(nd["model"].forward(x[:B], params), y[:B]).backward()
        nd["optimizer"].step()
    assert d_sgd._momentum_state(nodes) != "none"
    params["algorithm"]["device-training"] = True
    params["algorithm"]["device-training-gn-lenet"] = True
    with pytest.raises(ValueError, match="device-training-gn-lenet.*momentum"):
        d_sgd._trainer(nodes, state["topology"], params)


def test_evaluator_reads_the_trainers_slab(gpu):
    """Under both flags DeviceEvaluator reads the live trainer's slab in place and agrees with the
    float64 CPU loop."""
    from niidmix import d_sgd, evaluate
    params, nodes, topo, state = _setup("gn", evaluation=True)
    state, _, _, _ = d_sgd.next_step(state, params, None)
    x, y = _dataset()
    tests = [(x[i], int(y[i])) for i in range(N * S)]
    ev = evaluate.DeviceEvaluator(params).register_sets(test=tests)
    res = ev.accuracy(nodes, "test")
    assert ev.last_source == "trainer"
    own = ev.train_accuracy(nodes)
    assert ev.last_source == "trainer"
    d_sgd.synchronize()
    xs = torch.stack([s[0] for s in tests])
    ys = torch.tensor([s[1] for s in tests])
    for r, nd in enumerate(nodes):
        theta = torch.cat([q.detach().reshape(-1) for q in nd["model"].parameters()])
        for got, sl in ((res[r], slice(0, N * S)), (own[r], slice(r * S, (r + 1) * S))):
            z64 = th.forward_logits(theta, xs[sl], SHAPE[3], torch.float64)
            z32 = th.forward_logits(theta, xs[sl], SHAPE[3], torch.float32)
            e32 = float((z32.double() - z64).abs().max())
            nll = torch.logsumexp(z64, 1) - z64[torch.arange(z64.shape[0]), ys[sl]]
            top = z64.topk(2, dim=1).values
            amb = int(((top[:, 0] - top[:, 1]) <= 16 * e32).sum())
            correct = int((z64.argmax(1) == ys[sl]).sum())
            assert abs(got[0] * z64.shape[0] - correct) <= amb + 1e-9
            assert abs(got[1] - float(nll.mean())) <= 2 * 4 * e32
