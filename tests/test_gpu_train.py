"""--device-training on the GPU: the gradient kernel against float64, its layout and determinism
contracts, and the plugin's round -- its wiring bit for bit, seven rounds against the CPU path,
and a write between rounds."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

RTOL = 1e-5          # the project's fast-mode tolerance, on the condition-aware bound A


# ------------------------------------------------------------------------------------------------
# 1. the kernel against float64
#   name: (N rows, K, C, B, batch_len or None, weight scale, one label per batch, layout)
#   layout 'vec': ld = P rounded up to 4 (float4 paths where K allows); 'odd': ld = P + 3
CASES = {
    "784x10_b125": (3, 784, 10, 125, None, 1.0, False, "vec"),
    "784x10_b125_odd_ld": (3, 784, 10, 125, None, 1.0, False, "odd"),
    "784x10_b17": (2, 784, 10, 17, None, 1.0, False, "vec"),
    "5x3_b1": (1, 5, 3, 1, None, 1.0, False, "odd"),
    "1023x1024_b16": (2, 1023, 1024, 16, None, 1.0, False, "odd"),
    "33x7_short_batches": (4, 33, 7, 64, [64, 1, 63, 2], 1.0, False, "odd"),
    "784x10_b125_large_logits": (3, 784, 10, 125, None, 30.0, False, "vec"),
    "784x10_b17_one_label": (2, 784, 10, 17, None, 1.0, True, "vec"),
    "64x8_b20_float4": (2, 64, 8, 20, None, 1.0, False, "vec"),           # C % 4 == 0, B > 16
    "40x1024_b32_full_lds": (1, 40, 1024, 32, None, 1.0, False, "vec"),   # b_max * C = 32768
}
_cache = {}


def _ld(p, layout):
    return (p + 3) // 4 * 4 if layout == "vec" else p + 3


def _case(name):
    """Inputs and the float64 / float32 torch CPU references of a case, computed once."""
    if name in _cache:
        return _cache[name]
    from niidmix import train
    n, k, c, b, lens, scale, one_label, layout = CASES[name]
    gen = torch.Generator().manual_seed(len(name) * 7919 + n)
    torch.manual_seed(4321 + k + c)
    lens = lens or [b] * n
    s = n * b + 5
    x = torch.rand(s, k, generator=gen)
    y = torch.randint(0, c, (s,), generator=gen)
    idx = torch.stack([torch.randperm(s, generator=gen)[:b] for _ in range(n)])
    if one_label:
        for i in range(n):
            y[idx[i]] = (2 * i + 1) % c
    theta, g64, bound, l64, g32, l32 = [], [], [], [], [], []
    for i in range(n):
        fc = torch.nn.Linear(k, c)
        w, bias = (fc.weight.detach() * scale).clone(), fc.bias.detach().clone()
        theta.append(torch.cat([w.reshape(-1), bias]))
        xi, yi = x[idx[i, :lens[i]]], y[idx[i, :lens[i]]]
        l, g, a = train.fp64_reference(w, bias, xi, yi)
        l64.append(l), g64.append(g), bound.append(a)
        w32, b32 = w.clone().requires_grad_(), bias.clone().requires_grad_()
        loss = F.nll_loss(F.log_softmax(F.linear(xi.view(-1, k), w32, b32), 1), yi)
        loss.backward()
        g32.append(torch.cat([w32.grad.reshape(-1), b32.grad]))
        l32.append(loss.detach())
    out = dict(n=n, k=k, c=c, b=b, lens=lens, layout=layout, x=x, y=y, idx=idx,
               theta=torch.stack(theta), g64=torch.stack(g64), bound=torch.stack(bound),
               l64=torch.stack(l64), g32=torch.stack(g32), l32=torch.stack(l32))
    _cache[name] = out
    return out


def _launch(d, dev, rows=None, n_slab=None, theta=None, sentinel=0.0):
    """The op on a case: listed rows `rows` of an n_slab-row slab.  Returns (grad slab incl. its
    padding columns, loss)."""
    n, k, c = d["n"], d["k"], d["c"]
    p = c * k + c
    ld = _ld(p, d["layout"])
    rows = list(range(n))[::-1] if rows is None else rows
    n_slab = n_slab or n + 1
    th = torch.zeros(n_slab, ld, device=dev)
    src = d["theta"] if theta is None else theta
    for i, r in enumerate(rows):
        th[r, :p] = src[i].to(dev)
    grad = torch.full((n_slab, ld), sentinel, device=dev)
    loss = torch.zeros(n, device=dev)
    torch.ops.niidmix.linear_nll_grad_rows(
        th[:, :p], d["x"].to(dev), d["y"].to(torch.int32).to(dev),
        d["idx"].to(torch.int32).to(dev).contiguous(),
        torch.tensor(d["lens"], dtype=torch.int32, device=dev),
        torch.tensor(rows, dtype=torch.int32, device=dev), grad[:, :p], loss, k, c)
    torch.cuda.synchronize()
    return grad.cpu(), loss.cpu(), rows


def _worst(g, g64, bound):
    return float(((g.double() - g64).abs() / bound.clamp_min(1e-300)).max())


@pytest.mark.parametrize("name", list(CASES))
def test_kernel_against_float64(name, gpu):
    """|g - g64| <= 1e-5 A elementwise, A_W[c,k] = sum_s ((p64 + onehot) / len) |x[s,k]|, A_b[c] =
    sum_s (p64 + onehot) / len; |loss - loss64| <= 1e-5 max(|loss64|, 1).  torch's own fp32 CPU
    gradient must sit inside the same bound (else the inputs are wrong for this test)."""
    from niidmix import ops  # noqa: F401  (registers the op)
    d = _case(name)
    p = d["c"] * d["k"] + d["c"]
    r32 = _worst(d["g32"], d["g64"], d["bound"])
    assert r32 <= RTOL, f"torch fp32 outside the bound: {r32:.3g}"
    assert bool(((d["l32"].double() - d["l64"]).abs() <= RTOL * d["l64"].abs().clamp_min(1)).all())
    grad, loss, rows = _launch(d, gpu)
    g = torch.stack([grad[r, :p] for r in rows])
    rk = _worst(g, d["g64"], d["bound"])
    print(f"{name}: worst |g - g64| / A  kernel {rk:.3g}  torch fp32 {r32:.3g}")
    assert bool(((g.double() - d["g64"]).abs() <= RTOL * d["bound"]).all()), f"kernel {rk:.3g}"
    assert bool(((loss.double() - d["l64"]).abs() <= RTOL * d["l64"].abs().clamp_min(1)).all())


def test_rows_layout_and_determinism(gpu):
    """rows = [5, 0, 3] of an 8-row slab with ld = P + 3: unlisted rows and the 3 padding columns of
    grad keep the sentinel bit for bit, every element of a listed row is written, and a second
    launch gives the same bits."""
    from niidmix import ops  # noqa: F401
    d = dict(_case("33x7_short_batches"))
    d.update(n=3, lens=d["lens"][:3], idx=d["idx"][:3])
    p = d["c"] * d["k"] + d["c"]
    sentinel = 12345.678
    grad, loss, rows = _launch(d, gpu, rows=[5, 0, 3], n_slab=8, sentinel=sentinel)
    s = torch.tensor(sentinel)
    for r in range(8):
        if r in rows:
            assert not bool((grad[r, :p] == s).any()), f"row {r}: an element was not written"
            assert bool((grad[r, p:] == s).all()), f"row {r}: padding written"
        else:
            assert bool((grad[r] == s).all()), f"unlisted row {r} written"
    g = torch.stack([grad[r, :p] for r in rows])
    assert bool(((g.double() - d["g64"][:3]).abs() <= RTOL * d["bound"][:3]).all())
    grad2, loss2, _ = _launch(d, gpu, rows=[5, 0, 3], n_slab=8, sentinel=sentinel)
    assert torch.equal(grad, grad2) and torch.equal(loss, loss2)
    for name in ("784x10_b125", "1023x1024_b16"):
        a, b = _launch(_case(name), gpu), _launch(_case(name), gpu)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), name


def test_inf_weight_stays_in_its_row(gpu):
    from niidmix import ops  # noqa: F401
    d = _case("784x10_b17")
    p = d["c"] * d["k"] + d["c"]
    theta = d["theta"].clone()
    theta[1, 3] = float("inf")
    grad, loss, rows = _launch(d, gpu, theta=theta)
    assert not bool(torch.isfinite(loss[1])) and bool(torch.isfinite(loss[0]))
    g0 = grad[rows[0], :p]
    assert bool(((g0.double() - d["g64"][0]).abs() <= RTOL * d["bound"][0]).all())
    assert abs(float(loss[0]) - float(d["l64"][0])) <= RTOL * max(abs(float(d["l64"][0])), 1)


# ------------------------------------------------------------------------------------------------
# 2. the plugin's round: a 16-node ring, Linear(784, 10), batch 25
N, K, C, B, S = 16, 784, 10, 25, 100
LR = 0.1


class Net(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.fc = torch.nn.Linear(K, C)

    def forward(self, x, params):
        return F.log_softmax(self.fc(x.view(-1, K)), dim=1)


def _ring():
    w = torch.zeros(N, N)
    for i in range(N):
        for j in (i - 1, i, i + 1):
            w[i, j % N] = 1.0 / 3.0
    return {"edges": {i: [(i - 1) % N, (i + 1) % N] for i in range(N)}, "weights": w}


_data = {}


def _dataset():
    if not _data:
        g = torch.Generator().manual_seed(99)
        # sparse images (5 % of the pixels lit, |x|^2 ~ 13): plain SGD at lr 0.1 is stable on them
        x = torch.rand(N * S, 1, 28, 28, generator=g) * (torch.rand(N * S, 1, 28, 28, generator=g) < 0.05)
        y = (x.view(N * S, K) @ torch.randn(K, C, generator=g)).argmax(1)
        _data.update(x=x, y=y)
    return _data["x"], _data["y"]


def _setup(device_training, momentum=0.0):
    from niidmix import d_sgd
    torch.manual_seed(2024)
    params = {"meta": {"log": "WARNING", "seed": 2024}, "model": {"input-size": K},
              "topology": {"name": "ring", "remove-clique-edges": 0},
              "logger": {"accuracy-logging-interval": 0, "accuracy-logging-interval-steps": 0,
                         "log-consensus-distance": False},
              "algorithm": {"learning-rate": LR, "learning-momentum": momentum, "batch-size": B,
                            "initial-averaging": False, "clique-gradient": False,
                            "unbiased-gradient": False, "deferred-writeback": False,
                            "mixing-mode": "exact"}}
    if device_training:
        params["algorithm"]["device-training"] = True
    x, y = _dataset()
    nodes = []
    for r in range(N):
        mdl = Net()
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
    """mix(step(theta, g_kernel)): the op on the same indices, the existing step op (a first
    momentum step when momentum != 0), the oracle's reference loop for the mixing."""
    from niidmix import model as nm, train
    x, y = _dataset()
    p = C * K + C
    th = torch.zeros(N, train.padded_ld(p), device=dev)[:, :p]
    th.copy_(theta)
    grad = torch.zeros(N, train.padded_ld(p), device=dev)[:, :p]
    bi = torch.zeros(N, B, dtype=torch.int32)
    for i, idx in enumerate(batches):
        bi[i, :idx.numel()] = (idx + i * S).to(torch.int32)
    bl = torch.tensor([b.numel() for b in batches], dtype=torch.int32, device=dev)
    rows = torch.arange(N, dtype=torch.int32, device=dev)
    loss = torch.empty(N, device=dev)
    torch.ops.niidmix.linear_nll_grad_rows(th, x.view(N * S, K).to(dev), y.to(torch.int32).to(dev),
                                           bi.to(dev), bl, rows, grad, loss, K, C)
    if momentum:
        buf = torch.zeros(N, train.padded_ld(p), device=dev)[:, :p]
        torch.ops.niidmix.sgd_momentum_step_rows(th, grad, buf, rows, -LR, momentum, True)
    else:
        torch.ops.niidmix.sgd_step_rows(th, grad, rows, -LR)
    stepped = th.cpu()
    for i, nd in enumerate(nodes):
        nm.unflatten_into(nd["model"], stepped[i])
    oracle_mod.reference_loop_average(nodes, topo)
    return _flat(nodes), loss.cpu()


@pytest.mark.parametrize("momentum", [0.0, 0.9])
def test_one_round_equals_its_parts(momentum, gpu, oracle_mod):
    """After one --device-training next_step the models equal, bit for bit, mix(step(theta,
    g_kernel)) put together from a direct call of the op on the same indices, the existing step op
    and the oracle's reference_loop_average."""
    from niidmix import d_sgd, train
    params, nodes, topo, state = _setup(True, momentum)
    state, losses, _, active = d_sgd.next_step(state, params, None)
    d_sgd.synchronize()
    got = _flat(nodes)
    assert active is nodes and sorted(losses) == list(range(N))
    assert all(isinstance(v, float) for v in losses.values())

    params2, twin, topo2, _ = _setup(True, momentum)              # same seed: same models, same RNG
    theta0 = _flat(twin)
    batches, _ = train.draw(twin, params2)
    want, loss = _parts_round(theta0, batches, topo2, twin, momentum, gpu, oracle_mod)
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    assert [losses[r] for r in range(N)] == loss.tolist()


def test_seven_rounds_against_the_cpu_path(gpu):
    """(a) flag off, (b) the same rounds in float64 torch with a dense W^T theta mixing, (c) flag
    on; same seed, hence the same indices.  max|theta_c - theta_b| <= 10 max|theta_a - theta_b|:
    the yardstick is the reference's own fp32 drift, x10 for another summation order."""
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

    th_a, loss_a, done_a = run(False)
    th_c, loss_c, done_c = run(True)

    params, nodes, topo, _ = _setup(True)
    x, y = _dataset()
    x = x.view(N * S, K)
    th = _flat(nodes).double()
    wt = topo["weights"].double().t()
    for _ in range(rounds):
        batches, _ = train.draw(nodes, params)
        for i, idx in enumerate(batches):
            w, b = th[i, :C * K].view(C, K), th[i, C * K:]
            _, g, _ = train.fp64_reference(w, b, x[idx + i * S], y[idx + i * S])
            th[i] -= LR * g
        th = wt @ th
    drift_a = float((th_a.double() - th).abs().max())
    drift_c = float((th_c.double() - th).abs().max())
    print(f"seven rounds: max|theta_a - theta_b| {drift_a:.3g}  max|theta_c - theta_b| {drift_c:.3g}")
    assert drift_c <= 10 * drift_a
    mean = [sum(ls) / N for ls in loss_c]
    assert mean[-1] < mean[0]
    assert all(abs(c - a) <= 1e-5 * abs(a) for a, c in zip(loss_a[0], loss_c[0]))
    assert done_a == done_c and any(any(d.values()) for d in done_c)


def test_a_write_between_rounds(gpu, oracle_mod):
    """p.data.add_(1) on one node, then d_sgd.invalidate([node]): the next round starts from the
    written value (uploaded again), here checked bit for bit against the round put together from
    its parts."""
    from niidmix import d_sgd, train
    params, nodes, topo, state = _setup(True)
    state, _, _, _ = d_sgd.next_step(state, params, None)
    tr = d_sgd._trainers[id(nodes)]
    assert tr.param_uploads == 1
    state, _, _, _ = d_sgd.next_step(state, params, None)
    assert tr.param_uploads == 1                                   # resident between rounds
    with torch.no_grad():
        nodes[3]["model"].fc.weight.data.add_(1)
    d_sgd.invalidate([nodes[3]])
    written = _flat(nodes)
    state, _, _, _ = d_sgd.next_step(state, params, None)
    assert tr.param_uploads == 2
    got = _flat(nodes)

    params2, twin, topo2, _ = _setup(True)
    for _ in range(2):
        train.draw(twin, params2)
    batches, _ = train.draw(twin, params2)
    want, _ = _parts_round(written, batches, topo2, twin, 0.0, gpu, oracle_mod)
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))
