"""--learning-momentum on the device: k_sgd_momentum_step_rows against torch.optim.SGD on CPU
tensors, and the drop-in's resident rounds with momentum (plain and gradient-averaged) against the
CPU optimizer plus the reference mixing loop, bit for bit, including the hand-over of the
optimizer state between CPU and device steps."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

I32 = torch.int32


def _same_bits(a, b):
    """a == b bit for bit where the reference b is finite; NaN where it is NaN, the same
    infinity where it is infinite."""
    a, b = a.reshape(-1), b.reshape(-1)
    fin = torch.isfinite(b)
    return (a.shape == b.shape and torch.equal(a[fin].view(I32), b[fin].view(I32))
            and torch.equal(torch.isnan(a[~fin]), torch.isnan(b[~fin]))
            and torch.equal(a[~fin][~torch.isnan(b[~fin])], b[~fin][~torch.isnan(b[~fin])]))


# ------------------------------------------------------------------------------------------------
# 1. the kernel
SPECIALS = [-0.0, 0.0, float("inf"), float("-inf"), float("nan")]
ROWS = [0, 2, 5]


def _plant(t, gen):
    """A handful of -0.0, +0.0, inf, -inf and NaN at random places of every row."""
    for r in range(t.shape[0]):
        idx = torch.randperm(t.shape[1], generator=gen)[:2 * len(SPECIALS)]
        t[r, idx] = torch.tensor(SPECIALS * 2)


@pytest.mark.parametrize("shape,m,lr", [("scalar", 0.9, 0.07), ("vec4_ld", 0.9, 0.07),
                                        ("scalar", 0.95, 0.002)])
def test_momentum_step_kernel_bitwise(shape, m, lr, gpu):
    """Three consecutive steps (first, then two steady-state ones) of rows [0, 2, 5] of 6 equal
    torch.optim.SGD(momentum=m) on CPU tensors in p and in the momentum buffer; the other rows
    keep their parameters and the buffer's sentinel.  scalar: [6, 1003] contiguous (V = 1);
    vec4_ld: [6, 1032] column views of [6, 1040] tensors (float4 lanes, ld > ncols), whose
    columns outside the view must stay untouched too."""
    from niidmix import ops
    gen = torch.Generator().manual_seed(5)
    ncols, wide = (1003, 1003) if shape == "scalar" else (1032, 1040)
    off = {"p": 0, "g": 0, "buf": 0} if shape == "scalar" else {"p": 4, "g": 0, "buf": 8}
    p0 = torch.randn(6, ncols, generator=gen)
    _plant(p0, gen)
    dev = {k: torch.full((6, wide), s, device=gpu) for k, s in (("p", 3.0), ("g", 5.0), ("buf", 7.0))}
    view = {k: dev[k][:, off[k]:off[k] + ncols] for k in dev}
    view["p"].copy_(p0)
    rows = torch.tensor(ROWS, dtype=I32, device=gpu)
    ref = {r: torch.nn.Parameter(p0[r].clone()) for r in ROWS}
    opt = {r: torch.optim.SGD([ref[r]], lr=lr, momentum=m) for r in ROWS}
    for step in range(3):
        g = torch.randn(6, ncols, generator=gen)
        if step == 0:
            _plant(g, gen)
        view["g"].copy_(g)
        ops.sgd_momentum_step_rows(view["p"], view["g"], view["buf"], rows, -lr, m, step == 0)
        got_p, got_b = view["p"].cpu(), view["buf"].cpu()
        for r in range(6):
            if r in ROWS:
                ref[r].grad = g[r].clone()
                opt[r].step()
                assert _same_bits(got_p[r], ref[r].detach()), (step, r)
                assert _same_bits(got_b[r], opt[r].state[ref[r]]["momentum_buffer"]), (step, r)
            else:
                assert torch.equal(got_p[r].view(I32), p0[r].view(I32)), (step, r)
                assert bool((got_b[r] == 7.0).all()), (step, r)
    if shape != "scalar":                       # nothing written outside the column views
        for k, s in (("p", 3.0), ("buf", 7.0)):
            full = dev[k].cpu()
            assert bool((full[:, :off[k]] == s).all()) and bool((full[:, off[k] + ncols:] == s).all())


# ------------------------------------------------------------------------------------------------
# 2. argument checks through the C ABI
def test_momentum_step_argument_checks(gpu):
    from niidmix import _lib
    lib = _lib.lib
    assert hasattr(lib, "niidmix_sgd_momentum_step_rows_f32")
    assert lib.niidmix_abi_version() == 6
    p, g, buf = (torch.zeros(6, 1003, device=gpu) for _ in range(3))
    rows = torch.tensor(ROWS, dtype=I32, device=gpu)

    def call(pp, gg, bb, ld_b=1003):
        return lib.niidmix_sgd_momentum_step_rows_f32(
            pp, 1003, gg, 1003, bb, ld_b, 1003, rows.data_ptr(), 3, -0.07, 0.9, 0,
            ctypes.c_void_p(torch.cuda.current_stream(gpu).cuda_stream))

    for bb, ld_b, want in ((p.data_ptr(), 1003, _lib.EALIAS), (g.data_ptr(), 1003, _lib.EALIAS),
                           (None, 1003, _lib.EINVAL), (buf.data_ptr(), 1002, _lib.EINVAL)):
        assert call(p.data_ptr(), g.data_ptr(), bb, ld_b) == want
        assert lib.niidmix_last_error() != b""
    # partial overlap over the extent three rows imply: buf starts inside p's third row
    assert call(p.data_ptr(), g.data_ptr(), p.data_ptr() + 4 * (2 * 1003 + 1000)) == _lib.EALIAS
    assert call(p.data_ptr(), g.data_ptr(), buf.data_ptr()) == _lib.OK
    torch.cuda.synchronize()
    assert not bool(p.any()) and not bool(buf.any())


# ------------------------------------------------------------------------------------------------
# 3-6. the drop-in rounds: 4 nodes of Linear(784, 10) on a 4-node graph
class Net(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.fc = torch.nn.Linear(784, 10)

    def forward(self, x, params):
        return torch.nn.functional.log_softmax(self.fc(x.view(-1, 784)), dim=1)


W1 = [[0.5, 0.25, 0.0, 0.25], [0.25, 0.5, 0.25, 0.0], [0.0, 0.25, 0.5, 0.25], [0.25, 0.0, 0.25, 0.5]]
W2 = [[0.4, 0.3, 0.0, 0.3], [0.3, 0.4, 0.3, 0.0], [0.0, 0.3, 0.4, 0.3], [0.3, 0.0, 0.3, 0.4]]


def _topology(w):
    return {"edges": {0: [1, 3], 1: [0, 2], 2: [3, 1], 3: [2, 0]}, "weights": torch.tensor(w),
            "cliques": [[1, 0], [2, 3]],
            "neighbourhoods": {0: [0, 2], 1: [3, 1, 0], 2: [2], 3: [1, 3]}}


def _setup(alg, deferred, momentum=0.9):
    from niidmix import d_sgd
    torch.manual_seed(1337)
    params = {"meta": {"log": "WARNING", "seed": 1337}, "model": {"input-size": 784},
              "topology": {"name": "d-cliques" if alg else "ring", "remove-clique-edges": 0},
              "logger": {"accuracy-logging-interval": 0, "accuracy-logging-interval-steps": 0,
                         "log-consensus-distance": False},
              "algorithm": {"learning-rate": 0.1, "learning-momentum": momentum, "batch-size": 50,
                            "initial-averaging": False, "clique-gradient": alg == "clique",
                            "unbiased-gradient": alg == "unbiased",
                            "deferred-writeback": deferred}}
    g = torch.Generator().manual_seed(11)
    data = [(torch.rand(1, 28, 28, generator=g), int(torch.randint(0, 10, (1,), generator=g)))
            for _ in range(800)]
    nodes = []
    for r in range(4):
        mdl = Net()
        nodes.append({"rank": r, "epoch": 0, "train-set": data[r * 200:(r + 1) * 200],
                      "model": mdl, "optimizer": d_sgd.optimizer(mdl, params)})
    return params, nodes


def _flat(nodes, what):
    out = []
    for nd in nodes:
        qs = list(nd["model"].parameters())
        if what == "param":
            ts = [q.detach() for q in qs]
        elif what == "grad":
            ts = [q.grad.detach() for q in qs]
        else:
            ts = [nd["optimizer"].state[q]["momentum_buffer"] for q in qs]
        out.append(torch.cat([t.reshape(-1) for t in ts]))
    return torch.stack(out).clone()


def _run(alg, plan, monkeypatch, oracle_mod, deferred=False, after=None, topologies=None):
    """len(plan) rounds of next_step; plan[k] is how round k steps: 'device' (the resident device
    step / fused round), 'cpu' (NIIDMIX_DEVICE_STEP=0, with gradient averaging NIIDMIX_FUSED=0:
    the plugin's CPU optimizer step around its GPU kernels) or 'oracle' (every round: torch CPU
    ops only, the reference loops).  after(k, nodes): called after round k.  topologies: {round:
    weights} swaps the graph before that round.  Returns per-round parameters [4, P], the final
    gradients, the engines of every round and the nodes."""
    from niidmix import d_sgd
    monkeypatch.setenv("NIIDMIX_ROW_BLOCK", "3")
    params, nodes = _setup(alg, deferred)
    topo = _topology(W1)

    def cpu_gradient(nds, t, p):                  # d_sgd.py:47-94 restated with torch CPU ops
        if alg is None:
            stepped = range(len(nds))
        else:
            with torch.no_grad():
                if alg == "clique":
                    oracle_mod.reference_loop_clique_gradient(nds, t["cliques"])
                    stepped = [r for c in t["cliques"] for r in c]
                else:
                    hoods = t["neighbourhoods"]
                    grads = {n["rank"]: d_sgd.average_gradients([nds[q]["model"]
                                                                 for q in hoods[n["rank"]]])
                             for n in nds}
                    for n in nds:
                        d_sgd.update_gradients([n["model"]], grads[n["rank"]])
                    stepped = [n["rank"] for n in nds]
        for r in stepped:
            nds[r]["optimizer"].step()

    oracle = plan[0] == "oracle"
    saved = d_sgd.gradient, d_sgd.average, d_sgd._row_streamed
    if oracle:
        d_sgd.gradient = cpu_gradient
        d_sgd.average = lambda nds, t, p: oracle_mod.reference_loop_average(nds, t)
        d_sgd._row_streamed = lambda p: False
    snaps, engines = [], []
    try:
        state, _, _ = d_sgd.init(nodes, topo, params)
        for k, how in enumerate(plan):
            on = "1" if how == "device" else "0"
            monkeypatch.setenv("NIIDMIX_DEVICE_STEP", on)
            monkeypatch.setenv("NIIDMIX_FUSED", on)
            if topologies and k in topologies:
                state["topology"] = _topology(topologies[k])
            state, _, _, _ = d_sgd.next_step(state, params, None)
            eng = d_sgd.round_engine(nodes)
            engines.append(eng)
            if how == "device" and deferred:
                assert eng.resident.pending       # next_step returned before the write-back
            d_sgd.synchronize()
            snaps.append(_flat(nodes, "param"))
            if after is not None:
                after(k, nodes)
    finally:
        d_sgd.gradient, d_sgd.average, d_sgd._row_streamed = saved
    return snaps, _flat(nodes, "grad"), engines, nodes


_refs = {}


def _reference(alg, monkeypatch, oracle_mod):
    """The all-CPU run (computed once per variant, never modified): per-round parameters and
    momentum buffers of 6 rounds, and the gradients left after round 5."""
    if alg not in _refs:
        bufs, grads = [], {}

        def after(k, nodes):
            bufs.append(_flat(nodes, "buf"))
            if k == 4:
                grads[4] = _flat(nodes, "grad")
        snaps, _, _, _ = _run(alg, ["oracle"] * 6, monkeypatch, oracle_mod, after=after)
        _refs[alg] = (snaps, bufs, grads[4])
    return _refs[alg]


def _assert_rounds(got, ref):
    for k, (u, v) in enumerate(zip(got, ref)):
        assert _same_bits(u, v), f"round {k}"


@pytest.mark.parametrize("deferred", [False, True])
def test_plain_round_with_momentum(deferred, gpu, oracle_mod, monkeypatch):
    """Plain D-SGD with learning-momentum 0.9, 6 rounds, exact mode: the device step, the CPU step
    (NIIDMIX_DEVICE_STEP=0) and the pure CPU loop (optimizer.step() + the reference mixing) agree
    in every parameter bit after every round.  The device run takes the resident device-step
    engine, uploads the parameters once, and keeps one [N, w] momentum buffer per stripe."""
    from niidmix import d_sgd
    ref, _, _ = _reference(None, monkeypatch, oracle_mod)
    dev, _, engines, nodes = _run(None, ["device"] * 6, monkeypatch, oracle_mod, deferred=deferred)
    eng = engines[-1]
    assert isinstance(eng, d_sgd._FusedEngine) and eng.plain and eng.param_uploads == 1
    assert all(e is eng for e in engines)
    assert [tuple(pt["mbuf"].shape) for pt in eng.resident.parts] == [(4, 7850)]
    _assert_rounds(dev, ref)
    cpu, _, engines, _ = _run(None, ["cpu"] * 6, monkeypatch, oracle_mod, deferred=deferred)
    assert isinstance(engines[-1], d_sgd._Engine)
    _assert_rounds(cpu, ref)


@pytest.mark.parametrize("alg", ["clique", "unbiased"])
def test_gradient_averaging_with_momentum(alg, gpu, oracle_mod, monkeypatch):
    """--clique-gradient / --unbiased-gradient with learning-momentum 0.9, 5 rounds: the fused
    resident round (gradient mean, momentum step, mixing on the device) equals the unfused path
    (NIIDMIX_FUSED=0: GPU gradient mean, CPU optimizer step, GPU mixing) and the CPU reference
    loops, in every parameter bit of every round and in the gradients written back."""
    from niidmix import d_sgd
    ref, _, ref_grad = _reference(alg, monkeypatch, oracle_mod)
    fused, grad, engines, _ = _run(alg, ["device"] * 5, monkeypatch, oracle_mod)
    eng = engines[-1]
    assert isinstance(eng, d_sgd._FusedEngine) and not eng.plain and eng.resident is not None
    assert eng.momentum == 0.9 and "mbuf" in eng.resident.parts[0]
    _assert_rounds(fused, ref[:5])
    assert _same_bits(grad, ref_grad)
    unfused, grad, _, nodes = _run(alg, ["cpu"] * 5, monkeypatch, oracle_mod)
    assert (id(nodes), False) not in d_sgd._fused_engines
    _assert_rounds(unfused, ref[:5])
    assert _same_bits(grad, ref_grad)
    deferred, grad, _, _ = _run(alg, ["device"] * 5, monkeypatch, oracle_mod, deferred=True)
    _assert_rounds(deferred, ref[:5])
    assert _same_bits(grad, ref_grad)


@pytest.mark.parametrize("alg", [None, "clique"])
def test_handover_device_to_cpu(alg, gpu, oracle_mod, monkeypatch):
    """3 device rounds, sync_optimizer_state: every optimizer holds the momentum_buffer the
    all-CPU run holds after 3 rounds, as plain per-parameter tensors.  Then 2 rounds of CPU steps
    with no further sync call (the plugin exports on the switch): the all-CPU run's 5 rounds."""
    from niidmix import d_sgd
    ref, ref_buf, _ = _reference(alg, monkeypatch, oracle_mod)

    def after(k, nodes):
        if k == 2:
            d_sgd.sync_optimizer_state(nodes)
            assert _same_bits(_flat(nodes, "buf"), ref_buf[2])
            for nd in nodes:
                for q in nd["model"].parameters():
                    b = nd["optimizer"].state[q]["momentum_buffer"]
                    assert b.shape == q.shape and b.is_contiguous() and not b.is_pinned()
                    assert b.untyped_storage().nbytes() == 4 * q.numel()
    got, _, engines, nodes = _run(alg, ["device"] * 3 + ["cpu"] * 2, monkeypatch, oracle_mod,
                                  after=after)
    assert isinstance(engines[2], d_sgd._FusedEngine)
    assert (id(nodes), alg is None) not in d_sgd._fused_engines     # dropped on the switch
    _assert_rounds(got, ref[:5])
    assert _same_bits(_flat(nodes, "buf"), ref_buf[4])


def test_handover_needs_no_sync_call(gpu, oracle_mod, monkeypatch):
    """Device rounds, then CPU rounds, with no sync_optimizer_state call at all."""
    ref, ref_buf, _ = _reference(None, monkeypatch, oracle_mod)
    got, _, _, nodes = _run(None, ["device"] * 2 + ["cpu"] * 2, monkeypatch, oracle_mod)
    _assert_rounds(got, ref[:4])
    assert _same_bits(_flat(nodes, "buf"), ref_buf[3])


@pytest.mark.parametrize("alg", [None, "clique"])
def test_handover_cpu_to_device(alg, gpu, oracle_mod, monkeypatch):
    """2 rounds of CPU steps, then 3 device rounds: the new engine adopts the optimizers'
    momentum buffers (its first device step is not a `first` step) and the run equals the all-CPU
    run's 5 rounds; the exported state equals its buffers."""
    from niidmix import d_sgd
    ref, ref_buf, _ = _reference(alg, monkeypatch, oracle_mod)
    got, _, engines, nodes = _run(alg, ["cpu"] * 2 + ["device"] * 3, monkeypatch, oracle_mod)
    assert isinstance(engines[4], d_sgd._FusedEngine) and engines[4] is engines[2]
    _assert_rounds(got, ref[:5])
    d_sgd.sync_optimizer_state()
    assert _same_bits(_flat(nodes, "buf"), ref_buf[4])


def test_momentum_survives_topology_swap(gpu, oracle_mod, monkeypatch):
    """A new graph between two device rounds (random-graph --randomize: _FusedEngine.set_topology):
    the same engine, the same momentum buffer, parameters uploaded once, and the run equals the
    CPU run with the same swap."""
    from niidmix import d_sgd
    swap = {2: W2, 3: W1}
    ref, _, _, _ = _run(None, ["oracle"] * 4, monkeypatch, oracle_mod, topologies=swap)
    ptrs = []
    got, _, engines, _ = _run(
        None, ["device"] * 4, monkeypatch, oracle_mod, topologies=swap,
        after=lambda k, nodes: ptrs.append(
            d_sgd.round_engine(nodes).resident.parts[0]["mbuf"].data_ptr()))
    assert all(e is engines[0] for e in engines) and engines[0].param_uploads == 1
    assert len(set(ptrs)) == 1
    _assert_rounds(got, ref)
    assert not _same_bits(ref[3], _reference(None, monkeypatch, oracle_mod)[0][3])   # the swap matters


def test_invalidate_keeps_momentum(gpu, oracle_mod, monkeypatch):
    """invalidate() between device rounds re-uploads the parameters only: the momentum buffer
    stays, and the run still equals the all-CPU run."""
    from niidmix import d_sgd
    ref, _, _ = _reference(None, monkeypatch, oracle_mod)
    got, _, engines, _ = _run(None, ["device"] * 4, monkeypatch, oracle_mod,
                              after=lambda k, nodes: d_sgd.invalidate(nodes) if k == 1 else None)
    assert engines[-1].param_uploads == 2 and all(e is engines[0] for e in engines)
    _assert_rounds(got, ref[:4])


@pytest.mark.parametrize("stripes", [1, 2])
def test_plain_round_with_momentum_stripes(stripes, gpu, oracle_mod, monkeypatch):
    """The plain momentum round with NIIDMIX_DEVICES naming this GPU once, and twice with the
    parameter columns split into two stripes (each with its own momentum buffer): the all-CPU
    run, bit for bit, and the exported optimizer state assembled from both stripes."""
    from niidmix import d_sgd, slab
    ref, ref_buf, _ = _reference(None, monkeypatch, oracle_mod)
    monkeypatch.setenv("NIIDMIX_DEVICES", ",".join(["0"] * stripes))
    monkeypatch.setattr(slab, "MIN_STRIPE_COLS", 2048)
    got, _, engines, nodes = _run(None, ["device"] * 4, monkeypatch, oracle_mod)
    eng = engines[-1]
    assert isinstance(eng, d_sgd._FusedEngine) and eng.plain
    assert [pt["mbuf"].shape[1] for pt in eng.resident.parts] == ([7850] if stripes == 1 else
                                                                 [4096, 3754])
    _assert_rounds(got, ref[:4])
    d_sgd.sync_optimizer_state(nodes)
    assert _same_bits(_flat(nodes, "buf"), ref_buf[3])
