"""niidmix.family, the parts that need no GPU: GN-LeNet's one table and its views, the kernel
limits (one definition, seen by the host refusals and by the ops alike), the argument checks the
two gradient ops and the two evaluation ops share, and the one cut of a call's job list."""
import pytest
import torch

import test_eval_gnlenet_host as th
import test_train_gnlenet_host as tt


class AsIfOnDevice(torch.Tensor):
    """A CPU tensor that calls itself a device tensor, so that the ops' shared argument checkers
    run past `expected a HIP (cuda) tensor` on a host without a GPU.  These go to the checkers
    (ops._grad_rows_args, ops._eval_rows_args) only, which launch nothing whatever they decide;
    the ops themselves are called with plain CPU tensors alone, which they always refuse."""
    is_cuda = property(lambda self: True)


def dev(*shape, dtype=torch.float32):
    return torch.zeros(*shape, dtype=dtype).as_subclass(AsIfOnDevice)


I32, I64, F64 = torch.int32, torch.int64, torch.float64


# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cin,c,hw", [(1, 10, (28, 28)), (3, 10, (32, 32)), (4, 7, (15, 15)),
                                      (2, 1024, (64, 64))])
def test_one_table_many_views(cin, c, hw):
    """The fixture shapes and both ends of every limit: the table's shapes are the module's, the
    offsets the running sum of its numel(), P and F those of ops.gnlenet_sizes, and a split row
    gives back each tensor's own slice."""
    from niidmix import family, ops
    ps = list(th.GNLeNet(cin, c, hw).parameters())
    f, p = ops.gnlenet_sizes(cin, hw[0], hw[1], c)
    assert (f, p) == th.sizes(cin, hw[0], hw[1], c)
    assert ops.gnlenet_shapes(cin, c, f) == [tuple(q.shape) for q in ps]
    off = family.gn_lenet_offsets(cin, c, f)
    run = [0]
    for q in ps:
        run.append(run[-1] + q.numel())
    assert off == run and off[-1] == p == family.GN_LENET.P((cin, c, f))
    assert f == ps[12].shape[1] and family.gn_lenet_shape(th.GNLeNet(cin, c, hw)) == (cin, c, f)
    parts = family.split_gn_lenet(torch.arange(p), cin, hw)
    assert len(parts) == 14
    for i, (t, q) in enumerate(zip(parts, ps)):
        assert t.shape == q.shape and torch.equal(t.reshape(-1), torch.arange(off[i], off[i + 1])), i


# ------------------------------------------------------------------------------------------------
def _gn_ops_refuse(cin, h, w, c):
    """Whether the two GN-LeNet ops refuse the shape as unsupported.  The limits are checked
    before any tensor is looked at, so plain CPU tensors do; a shape within the limits is refused
    for the CPU tensors instead (nothing is launched either way)."""
    from niidmix import ops
    z, zi = torch.zeros(1, 1), torch.zeros(1, dtype=I32)
    seen = []
    for call in (lambda: ops.gnlenet_nll_grad_rows(z, z, zi, zi, zi, zi, z, z, cin, h, w, c),
                 lambda: ops.gnlenet_eval_rows(z, z, zi, zi, zi, zi, 1, z, zi, None, None, cin, h, w, c)):
        with pytest.raises(RuntimeError) as e:
            call()
        seen.append("unsupported shape" in str(e.value))
        assert seen[-1] or "expected a HIP" in str(e.value)
    assert seen[0] == seen[1]
    return seen[0]


def test_limits_agree():
    """Each limit, at the limit and one past it, on the host side (check_eligible / sizes: a
    ValueError naming the flag) and on the op's side.  The GN-LeNet ops check their limits in
    Python; the linear ops leave C and batch-size * C to the C entry point, which is therefore the
    op's side here (made-up addresses, refused before they are dereferenced; at the limit the call
    is refused for its leading dimension, a check that comes after the limits)."""
    from niidmix import _lib, evaluate, family, ops, train
    L = _lib.lib
    gn, lin = family.GN_LENET, family.LINEAR
    max_c, max_bc = ops.MAX_C, ops.MAX_BC
    lo, hi, max_cin = ops.GN_MIN_HW, ops.GN_MAX_HW, ops.GN_MAX_CIN

    # C, GN-LeNet: the train and the evaluation refusal, and both ops
    p = tt._params()
    pe = th._params()
    assert train.check_eligible(tt._nodes(p, [th.GNLeNet(c=max_c)]), p) == (1, max_c, 256)
    assert evaluate.check_eligible(th._nodes(pe, [th.GNLeNet(c=max_c)]), pe) == (1, max_c, 256)
    with pytest.raises(ValueError, match="device-training-gn-lenet"):
        train.check_eligible(tt._nodes(p, [th.GNLeNet(c=max_c + 1)]), p)
    with pytest.raises(ValueError, match="device-evaluation"):
        evaluate.check_eligible(th._nodes(pe, [th.GNLeNet(c=max_c + 1)]), pe)
    assert not _gn_ops_refuse(1, 28, 28, max_c) and _gn_ops_refuse(1, 28, 28, max_c + 1)

    # Cin
    assert train.check_eligible(tt._nodes(p, [th.GNLeNet(cin=max_cin)], (max_cin, 28, 28)), p) == (max_cin, 10, 256)
    assert evaluate.check_eligible(th._nodes(pe, [th.GNLeNet(cin=max_cin)]), pe) == (max_cin, 10, 256)
    with pytest.raises(ValueError, match="device-training-gn-lenet"):
        train.check_eligible(tt._nodes(p, [th.GNLeNet(cin=max_cin + 1)], (max_cin + 1, 28, 28)), p)
    with pytest.raises(ValueError, match="device-evaluation"):
        evaluate.check_eligible(th._nodes(pe, [th.GNLeNet(cin=max_cin + 1)]), pe)
    assert not _gn_ops_refuse(max_cin, 28, 28, 10) and _gn_ops_refuse(max_cin + 1, 28, 28, 10)

    # H and W, both ends
    for h, w in ((lo, lo), (hi, hi), (lo, hi)):
        shape = (1, 10, ops.gnlenet_sizes(1, h, w, 10)[0])
        assert gn.sizes((1, h, w), shape, "--flag", "the set") == (1, h, w, 10)
        assert not _gn_ops_refuse(1, h, w, 10)
    for h, w in ((lo - 1, lo), (lo, lo - 1), (hi + 1, hi), (hi, hi + 1)):
        with pytest.raises(ValueError, match="--flag.*H, W"):
            gn.sizes((1, h, w), (1, 10, 64), "--flag", "the set")
        assert _gn_ops_refuse(1, h, w, 10)

    # C and batch-size * C, linear
    k = 6
    b = max_bc // max_c
    pl = tt._params(**{"batch-size": b})
    ple = th._params()
    assert train.check_eligible(th._nodes(pl, [th.Net(k, max_c)]), pl) == (k, max_c)
    assert evaluate.check_eligible(th._nodes(ple, [th.Net(k, max_c)]), ple) == (k, max_c)
    with pytest.raises(ValueError, match="device-training"):
        train.check_eligible(th._nodes(pl, [th.Net(k, max_c + 1)]), pl)
    with pytest.raises(ValueError, match="device-evaluation"):
        evaluate.check_eligible(th._nodes(ple, [th.Net(k, max_c + 1)]), ple)
    pl1 = tt._params(**{"batch-size": b + 1})
    with pytest.raises(ValueError, match="device-training.*batch-size"):
        train.check_eligible(th._nodes(pl1, [th.Net(k, max_c)]), pl1)
    lin.limits((k, max_c), "--flag", b)
    lin.limits((k, max_c), "--flag")

    def grad(c, b_max):            # ld_t = 1: too small, so that no call gets past its checks
        return L.niidmix_linear_nll_grad_rows_f32(1 << 20, 1, 8, 8, 8, 8, b_max, 8, 2, 1 << 30, 1, 8, k, c,
                                                  1 << 40, L.niidmix_linear_nll_grad_rows_scratch_elems(2, b_max, c), None)

    def ev(c):
        return L.niidmix_linear_eval_rows_f32(1 << 20, 1, 8, 8, 8, 8, 8, 2, 100, 1 << 30, (1 << 30) + 4096, None, 0,
                                              k, c, 1 << 40, L.niidmix_linear_eval_rows_scratch_bytes(2, 100, c), None)
    assert grad(max_c, b) == _lib.EINVAL and b"leading dimension" in L.niidmix_last_error()
    assert grad(max_c + 1, 1) == _lib.EUNSUPPORTED
    assert grad(max_c, b + 1) == _lib.EUNSUPPORTED and b"b_max * C" in L.niidmix_last_error()
    assert grad(3, max_bc // 3) == _lib.EINVAL and grad(3, max_bc // 3 + 1) == _lib.EUNSUPPORTED
    assert ev(max_c) == _lib.EINVAL and b"leading dimension" in L.niidmix_last_error()
    assert ev(max_c + 1) == _lib.EUNSUPPORTED


# ------------------------------------------------------------------------------------------------
N_ROWS, N_SAMPLES, B_MAX, MAX_LEN = 2, 7, 4, 3


def _pair(which):
    """Per member of a pair, linear then GN-LeNet, at small valid shapes: (op, its size arguments,
    what the op hands the pair's checker after the tensors)."""
    from niidmix import ops
    lin_p, gn_p = 3 * 5 + 3, ops.gnlenet_sizes(1, 15, 15, 1)[1]
    lin = (f"C * K + C = {lin_p}", lin_p, "K", 5)
    gn = (f"P = {gn_p}", gn_p, "Cin * H * W", 225)
    if which == "grad":
        return [(ops.linear_nll_grad_rows, (5, 3), lin + (False,)), (ops.gnlenet_nll_grad_rows, (1, 15, 15, 1), gn + (True,))]
    return [(ops.linear_eval_rows, (5, 3), (3,) + lin), (ops.gnlenet_eval_rows, (1, 15, 15, 1), (1,) + gn)]


def _plain(args):
    return [v.as_subclass(torch.Tensor) if isinstance(v, torch.Tensor) else v for v in args]


def _grad_args(p, cols, n=N_ROWS):
    return dict(theta=dev(N_ROWS, p), data=dev(N_SAMPLES, cols), labels=dev(N_SAMPLES, dtype=I32),
                batch_idx=dev(n, B_MAX, dtype=I32), batch_len=dev(n, dtype=I32), rows=dev(n, dtype=I32),
                grad=dev(N_ROWS, p), loss=dev(n))


def _eval_args(p, cols, n=N_ROWS):
    return dict(theta=dev(N_ROWS, p), data=dev(N_SAMPLES, cols), labels=dev(N_SAMPLES, dtype=I32),
                rows=dev(n, dtype=I32), seg_start=dev(n, dtype=I32), seg_len=dev(n, dtype=I32),
                max_len=MAX_LEN, loss_sum=dev(n, dtype=F64), correct=dev(n, dtype=I32), pred=None)


def _on(theta, dtype, *shape):
    """A tensor of `dtype` and `shape` on theta's first bytes."""
    flat = theta.as_subclass(torch.Tensor).reshape(-1).view(dtype)
    return flat[:int(torch.Size(shape).numel())].view(*shape).as_subclass(AsIfOnDevice)


def test_shared_validation_covers_both_families():
    """The cases of the four *_argument_errors_without_gpu tests, which put them to the C entry
    points as made-up addresses, restated as tensors (a null pointer becomes a tensor off the
    device or of another dtype, a short leading dimension a column short, an address inside theta
    a tensor on theta's storage): every case that both members of a pair take gets the same
    complaint for both, apart from how the column count is named.  The size arguments, which each
    op checks itself before anything else, go to the ops (plain CPU tensors); everything else goes
    to the pair's checker with what the member hands it."""
    import re
    from niidmix import ops
    for op, sizes, tail in _pair("grad"):
        p_text, p, _, cols, _ = tail

        def refused(match, **change):
            args = dict(_grad_args(p, cols), **change)
            with pytest.raises(RuntimeError, match=match):
                ops._grad_rows_args(*args.values(), *tail)
        for bad in ((0,) + sizes[1:], sizes[:-1] + (-1,)):
            with pytest.raises(RuntimeError, match=">= 1"):
                op(*_plain(_grad_args(p - 1, cols).values()), *bad)            # sizes before the slabs
        more = _grad_args(p, cols, n=N_ROWS + 1)
        del more["theta"], more["grad"], more["data"], more["labels"]
        assert ops._grad_rows_args(*_grad_args(p, cols).values(), *tail) == N_ROWS
        refused("theta: expected a HIP", theta=torch.zeros(N_ROWS, p))
        refused("grad: expected a HIP", grad=torch.zeros(N_ROWS, p))
        refused("data: expected a HIP", data=torch.zeros(N_SAMPLES, cols))
        refused("grad: expected float32", grad=dev(N_ROWS, p, dtype=F64))
        for name in ("labels", "batch_len", "rows"):
            refused(f"{name}: expected torch.int32", **{name: dev(N_SAMPLES, dtype=I64)})
        refused("loss: expected torch.float32", loss=dev(N_ROWS, dtype=F64))
        refused("batch_idx: expected a contiguous int32", batch_idx=dev(N_ROWS, B_MAX, dtype=I64))
        refused("batch_idx: expected a contiguous int32", batch_idx=dev(N_ROWS * B_MAX, dtype=I32))
        refused(re.escape(f"theta and grad: expected {p_text} columns, got {p - 1} and {p}"), theta=dev(N_ROWS, p - 1))
        refused(re.escape(f"theta and grad: expected {p_text} columns, got {p} and {p - 1}"), grad=dev(N_ROWS, p - 1))
        refused(f"data: expected {cols} columns", data=dev(N_SAMPLES, cols - 1))
        refused("data: expected a contiguous", data=dev(N_SAMPLES, cols + 1)[:, :cols])
        refused(f"labels: expected {N_SAMPLES} elements", labels=dev(N_SAMPLES - 1, dtype=I32))
        refused(f"batch_len: expected {N_ROWS} elements", batch_len=dev(N_ROWS + 1, dtype=I32))
        refused(f"loss: expected {N_ROWS} elements", loss=dev(N_ROWS + 1))
        refused("more rows listed", **more)
        refused("b_max must be >= 1", batch_idx=dev(N_ROWS, 0, dtype=I32))
        # the order: the slabs' columns, then the index tensors
        refused("theta and grad: expected", theta=dev(N_ROWS, p - 1), loss=dev(N_ROWS, dtype=F64))
        refused("labels: expected", labels=dev(1, dtype=I32), batch_idx=dev(N_ROWS, 0, dtype=I32))
        # the one difference inside the pair: only the GN-LeNet op refuses a grad or loss on theta
        args = _grad_args(p, cols)
        for change in (dict(grad=args["theta"]), dict(loss=_on(args["theta"], torch.float32, N_ROWS))):
            on_theta = list(dict(args, **change).values())
            assert ops._grad_rows_args(*on_theta, *tail[:-1], False) == N_ROWS
            with pytest.raises(RuntimeError, match="grad or loss overlaps theta"):
                ops._grad_rows_args(*on_theta, *tail[:-1], True)
    assert [t[2][-1] for t in _pair("grad")] == [False, True]

    for op, sizes, tail in _pair("eval"):
        _, p_text, p, _, cols = tail
        logits = (None,) if op is ops.gnlenet_eval_rows else ()

        def refused(match, **change):
            args = dict(_eval_args(p, cols), **change)
            with pytest.raises(RuntimeError, match=match):
                ops._eval_rows_args(*args.values(), None, *tail)
        for bad in ((0,) + sizes[1:], sizes[:-1] + (-1,)):
            with pytest.raises(RuntimeError, match=">= 1"):
                op(*_plain(_eval_args(p - 1, cols).values()), *logits, *bad)   # sizes before the slabs
        with pytest.raises(RuntimeError, match="max_len must be >= 0"):
            op(*_plain(dict(_eval_args(p, cols), max_len=-1).values()), *logits, *sizes)
        theta = dev(N_ROWS, p)
        assert ops._eval_rows_args(*_eval_args(p, cols).values(), None, *tail) == N_ROWS
        refused("theta: expected a HIP", theta=torch.zeros(N_ROWS, p))
        refused("data: expected a HIP", data=torch.zeros(N_SAMPLES, cols))
        for name in ("labels", "rows", "seg_start", "seg_len", "correct"):
            refused(f"{name}: expected torch.int32", **{name: dev(N_SAMPLES, dtype=I64)})
        refused("loss_sum: expected torch.float64", loss_sum=dev(N_ROWS))
        refused("rows: at least one job", rows=dev(0, dtype=I32))
        refused(re.escape(f"theta: expected {p_text} columns, got {p - 1}"), theta=dev(N_ROWS, p - 1))
        refused(f"data: expected {cols} columns", data=dev(N_SAMPLES, cols - 1))
        refused("data: expected a contiguous", data=dev(N_SAMPLES, cols + 1)[:, :cols])
        refused(f"labels: expected {N_SAMPLES} elements", labels=dev(N_SAMPLES - 1, dtype=I32))
        for name in ("seg_start", "seg_len", "correct"):
            refused(f"{name}: expected {N_ROWS} elements", **{name: dev(N_ROWS + 1, dtype=I32)})
        refused(f"loss_sum: expected {N_ROWS} elements", loss_sum=dev(N_ROWS + 1, dtype=F64))
        refused("pred: expected an int32", pred=dev(N_ROWS, MAX_LEN - 1, dtype=I32))
        refused("pred: expected an int32", pred=dev(N_ROWS + 1, MAX_LEN, dtype=I32))
        refused("an output overlaps theta", theta=theta, loss_sum=_on(theta, F64, N_ROWS))
        refused("an output overlaps theta", theta=theta, correct=_on(theta, I32, N_ROWS))
        refused("an output overlaps theta", theta=theta, pred=_on(theta, I32, N_ROWS, MAX_LEN))
        # the order: theta's columns, then the job list, then the outputs
        refused("theta: expected", theta=dev(N_ROWS, p - 1), pred=dev(N_ROWS, MAX_LEN - 1, dtype=I32))
        refused("pred: expected", theta=theta, pred=dev(N_ROWS, MAX_LEN - 1, dtype=I32),
                loss_sum=_on(theta, F64, N_ROWS))


# ------------------------------------------------------------------------------------------------
def test_cut_rows_is_the_only_cut(monkeypatch):
    """DeviceEvaluator cuts a GN-LeNet job list exactly as train.cut_rows cuts a row list, under
    a stubbed scratch size; a job that does not fit alone is a RuntimeError naming the flag; a
    linear job list is never cut."""
    from niidmix import evaluate, family, train
    sizes, max_len = (1, 28, 28, 10), 50
    asked = []

    def scratch(jobs, ml, sz):
        asked.append((ml, sz))
        return 1024 + 4096 * jobs * ml
    monkeypatch.setattr(family.GN_LENET, "eval_scratch_bytes", scratch)
    need = lambda k: 1024 + 4096 * k * max_len  # noqa: E731
    ev = evaluate.DeviceEvaluator({}, device="cpu")
    for n in (1, 2, 7, 1000):
        for fits, want in ((n, n), ((n + 1) // 2, (n + 1) // 2), (1, 1)):
            ev.scratch_budget = need(fits)
            got = ev._cut(family.GN_LENET, n, max_len, sizes, None)
            assert got == train.cut_rows(n, need, ev.scratch_budget) == want, (n, fits)
    assert asked and set(asked) == {(max_len, sizes)}
    ev.scratch_budget = need(1) - 1
    assert train.cut_rows(7, need, ev.scratch_budget) is None
    with pytest.raises(RuntimeError, match="device-evaluation"):
        ev._cut(family.GN_LENET, 7, max_len, sizes, None)
    monkeypatch.setattr(family.LINEAR, "eval_scratch_bytes", scratch)
    del asked[:]
    assert ev._cut(family.LINEAR, 1000, max_len, (784, 10), None) == 1000 and not asked
