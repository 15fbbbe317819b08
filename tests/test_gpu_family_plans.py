"""niidmix.family's plans on the GPU: a plan call is, bit for bit, the op it names called directly
on the same buffers -- gradient and loss for the gradient plans, loss_sum and correct for the
evaluation plans -- at the smallest shapes the kernels take.  Both sides run the same kernel on the
same inputs, so equality is exact."""
import pytest
import torch

pytestmark = pytest.mark.gpu

N_ROWS, N_SAMPLES, BATCH, JOB = 2, 7, 3, 5
SIZES = {"linear": (6, 4), "gn-lenet": (1, 15, 15, 3)}
_inputs = {}


def _family(kind):
    from niidmix import family
    return family.LINEAR if kind == "linear" else family.GN_LENET


def _case(kind, dev):
    """(theta [2, P] in a slab padded as the trainer's, data [7, *], labels [7]) of a family, made once."""
    if kind not in _inputs:
        from niidmix import ops, train
        sizes = SIZES[kind]
        p = 6 * 4 + 4 if kind == "linear" else ops.gnlenet_sizes(*sizes)[1]
        cols = 6 if kind == "linear" else 15 * 15
        g = torch.Generator().manual_seed(41)
        theta = torch.zeros(N_ROWS, train.padded_ld(p), device=dev)[:, :p]
        theta.copy_(0.1 * torch.randn(N_ROWS, p, generator=g))
        _inputs[kind] = (theta, torch.randn(N_SAMPLES, cols, generator=g).to(dev),
                         torch.randint(0, sizes[-1], (N_SAMPLES,), generator=g).to(torch.int32).to(dev))
    return _inputs[kind]


def _bits(t):
    return t.cpu().contiguous().view(torch.int32 if t.element_size() == 4 else torch.int64)


def _same(a, b):
    torch.cuda.synchronize()
    for x, y in zip(a, b):
        assert torch.equal(_bits(x), _bits(y))


def _grad_both(kind, b_max, want, dev, **switch):
    """The plan of grad_plan(sizes, b_max, **switch) against `want`, the op it must have bound: two
    jobs of BATCH samples in index blocks of b_max columns."""
    plan = _family(kind).grad_plan(SIZES[kind], b_max, **switch)
    assert plan.op is want and plan.b_max == b_max
    theta, data, labels = _case(kind, dev)
    bi = torch.zeros(N_ROWS, b_max, dtype=torch.int32)
    bi[:, :BATCH] = torch.tensor([[0, 1, 2], [6, 4, 3]], dtype=torch.int32)      # all < N_SAMPLES
    bi, bl = bi.to(dev), torch.full((N_ROWS,), BATCH, dtype=torch.int32, device=dev)
    rows = torch.tensor([1, 0], dtype=torch.int32, device=dev)

    def outs():
        return (torch.full((N_ROWS, theta.stride(0)), -7.0, device=dev)[:, :theta.shape[1]],
                torch.full((N_ROWS,), -7.0, device=dev))
    got, ref = outs(), outs()
    plan(theta, data, labels, bi, bl, rows, *got)
    want(theta, data, labels, bi, bl, rows, *ref, *SIZES[kind])
    _same(got, ref)
    assert bool(torch.isfinite(got[0]).all()) and bool(torch.isfinite(got[1]).all()) and bool((got[0] != -7).any())


def _eval_both(kind, want, kernel, dev, **switch):
    """The plan of eval_plan(sizes, **switch) against `want`: two jobs of JOB samples."""
    plan = _family(kind).eval_plan(SIZES[kind], **switch)
    assert plan.op is want and plan.kernel == kernel
    theta, data, labels = _case(kind, dev)
    rows, start, length = (torch.tensor(v, dtype=torch.int32, device=dev) for v in ([1, 0], [0, 2], [JOB, JOB]))
    assert int((start + length).max()) <= N_SAMPLES

    def outs():
        return (torch.full((N_ROWS,), -7.0, dtype=torch.float64, device=dev),
                torch.full((N_ROWS,), -7, dtype=torch.int32, device=dev))
    got, ref = outs(), outs()
    plan(theta, data, labels, rows, start, length, JOB, *got)
    want(theta, data, labels, rows, start, length, JOB, *ref, *([None] * (2 if plan.takes_logits else 1)),
         *SIZES[kind])
    _same(got, ref)
    assert bool((got[0] > 0).all()) and bool(((got[1] >= 0) & (got[1] <= JOB)).all())


def test_linear_plans_are_their_ops(gpu):
    from niidmix import ops
    _grad_both("linear", BATCH, ops.linear_nll_grad_rows, gpu)
    _grad_both("linear", BATCH, ops.linear_nll_grad_rows, gpu, large=True, mfma=True)
    # just over MAX_BC // C samples per index row: the sliced op is the one bound under the flag
    _grad_both("linear", ops.MAX_BC // 4 + 1, ops.linear_nll_grad_rows_sliced, gpu, large=True)
    _eval_both("linear", ops.linear_eval_rows, "k_lin_eval", gpu)
    _eval_both("linear", ops.linear_eval_rows, "k_lin_eval", gpu, mfma=True)


def test_gn_lenet_plans_are_their_ops(gpu, monkeypatch):
    from niidmix import family, ops
    monkeypatch.setattr(family.GN_LENET, "GRAD_MFMA_FASTER", {"map": True, "bands": True})
    monkeypatch.setattr(family.GN_LENET, "MFMA_FASTER", {4: True, 2: True})
    _grad_both("gn-lenet", BATCH, ops.gnlenet_nll_grad_rows, gpu)
    _grad_both("gn-lenet", BATCH, ops.gnlenet_nll_grad_rows, gpu, large=True)
    _grad_both("gn-lenet", BATCH, ops.gnlenet_nll_grad_rows_mfma, gpu, mfma=True)
    _eval_both("gn-lenet", ops.gnlenet_eval_rows, "k_gnl_eval", gpu)
    _eval_both("gn-lenet", ops.gnlenet_eval_rows_mfma, "k_gnl_eval_mfma", gpu, mfma=True)
