"""`-m gpu`: the four training-mode dense-block kernels per element against float64 of the same fp32 inputs (the bounds include/bcos_hip.h
states, evaluated by tests/densenet_train_emulation.py), their order / gate / bit contracts, and the fused DenseNet training plan against
the step recorded from the reference (tests/golden/densenet_tiny_train_step.*) and against the per-layer path.

Shapes: rows 1, 7, 256 (2 blocks of 128 rows), 257 (3 blocks of 86, 86 and 85 rows) and 4099 (33 blocks of 125 rows, the last one
short), and once 200704 = 64 x 56 x 56 (DenseNet-121's first block at batch 64: 1024 blocks of 196 rows, so that a lane walks more than
four rows and the finish kernels' four-chain loop over more than 48 blocks runs); C = 4 (one lane
per row), 32 (one channel tile), 72 and 260 (partial tiles; C / 4 not a divisor of 64: the looping form), 96 (three tiles); pitch C,
C + 4 and 1024 with the slice at offset 0, 4 and 8; NaN in every float around the slice and around the buffer.
The worst error / bound ratio of each kernel is printed (DESIGN.md section 3.5.1 records it)."""
import pytest
import torch

import densenet_emulation as DE
import densenet_train_cases as TC
import densenet_train_emulation as TE

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROWS = (1, 7, 256, 257, 4099)
CHANNELS = (4, 32, 72, 96, 260)
PAD = 64


@pytest.fixture(scope="module")
def lib(hip_lib):
    assert torch.cuda.is_available()
    return hip_lib


def _layouts(C):
    return ((C, 0), (C + 4, 4), (1024, 8))


def _pitched(values, pitch, off):
    """a NaN buffer on the device with `values` [rows, C] as the channel slice [off, off + C) of rows `pitch` floats apart, NaN floats
    in front of the first and behind the last row too -> (whole buffer, the slice)"""
    rows, C = values.shape
    flat = torch.full((rows * pitch + 2 * PAD,), float("nan"), device=DEV)
    sl = flat[PAD:PAD + rows * pitch].view(rows, pitch)[:, off:off + C]
    sl.copy_(values.to(DEV))
    return flat, sl


def _same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _only_slice_written(flat, sl, before=None):
    """every float of the buffer outside the slice is still NaN (`before`: and the whole buffer has the bits it had)"""
    if before is not None:
        return _same_bits(flat, before)
    mask = torch.ones_like(flat, dtype=torch.bool)
    rows, C = sl.shape
    pitch = sl.stride(0) if rows > 1 else C
    off = sl.storage_offset() - PAD
    idx = (off + torch.arange(rows, device=DEV)[:, None] * pitch + torch.arange(C, device=DEV)[None, :] + PAD).reshape(-1)
    mask[idx] = False
    return bool(flat[mask].isnan().all()) and not bool(flat[~mask].isnan().any())


def _inputs(rows, C, seed):
    """random columns of different spread and offset; from 7 rows on, channels 0..3 of the first rows hold inputs whose pre-activation
    x * g + shift rounds to +0, -0, the smallest normals and subnormals, and exact zeros"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(rows, C, generator=g) * (torch.rand(C, generator=g) * 4 + 0.05) + torch.randn(C, generator=g) * 3
    gvec = (torch.rand(C, generator=g) + 0.5) * torch.where(torch.rand(C, generator=g) < 0.25, -1.0, 1.0)
    shift = torch.randn(C, generator=g) * 0.5
    if rows >= 7:
        tiny, sub = 2.0 ** -126, 2.0 ** -149
        gvec[:4] = torch.tensor([0.5, 1.0, 0.5, 1.0])
        shift[:4] = torch.tensor([-1.0, 0.0, 0.0, tiny])
        x[:5, 0] = torch.tensor([2.0, 2.0 + 2.0 ** -22, 2.0 - 2.0 ** -22, -2.0, 0.0])
        x[:5, 1] = torch.tensor([tiny, -tiny, tiny / 2, -0.0, 0.0])
        x[:5, 2] = torch.tensor([tiny, sub, -sub, 3 * sub, -tiny])
        x[:5, 3] = torch.tensor([-tiny, -tiny / 2, -2 * tiny, sub - tiny, 0.0])
    d = (torch.rand(rows, C, generator=g) + 0.5) * torch.where(torch.rand(rows, C, generator=g) < 0.5, -1.0, 1.0)
    g_old = torch.randn(rows, C, generator=g)
    mean = x.mean(0) + torch.randn(C, generator=g) * 0.01
    coef = torch.randn(C, generator=g) * 0.1
    return x, gvec, shift, d, g_old, mean, coef


def _ratio(err, bound):
    return float((err / bound).max())


@pytest.mark.parametrize("C", CHANNELS)
def test_slice_batch_stats(lib, C):
    from bcos_hip import ops
    worst = 0.0
    for rows in ROWS:
        x = _inputs(rows, C, seed=rows + C)[0]
        m64, v64, bm, bv = TE.slice_batch_stats64(x)
        first = None
        for pitch, off in _layouts(C):
            flat, xs = _pitched(x, pitch, off)
            before = flat.clone()
            out = torch.full((2, C + 8), float("nan"), device=DEV)
            mean, var = ops.slice_batch_stats(xs, out[0, 4:C + 4], out[1, 4:C + 4])
            assert _only_slice_written(flat, xs, before), (rows, C, pitch)
            assert bool(out[:, :4].isnan().all()) and bool(out[:, C + 4:].isnan().all()), (rows, C, pitch)
            mean, var = mean.cpu(), var.cpu()
            assert not bool(mean.isnan().any() | var.isnan().any()), (rows, C, pitch)      # (a read outside the slice would have met a NaN)
            rm, rv = _ratio((mean.double() - m64).abs(), bm), _ratio((var.double() - v64).abs(), bv)
            worst = max(worst, rm, rv)
            assert rm <= 1.0 and rv <= 1.0, (rows, C, pitch, rm, rv)
            assert bool((var >= 0).all())
            if first is None:
                first = (mean, var)
                again = ops.slice_batch_stats(xs, torch.empty(C, device=DEV), torch.empty(C, device=DEV))
                assert torch.equal(again[0].cpu(), mean) and torch.equal(again[1].cpu(), var), (rows, C)      # the same state twice
            else:                                                                                            # ... and whatever the pitch / offset
                assert torch.equal(mean, first[0]) and torch.equal(var, first[1]), (rows, C, pitch)
    print(f"bcos_slice_batch_stats C={C}: worst error / bound {worst:.3g}")


@pytest.mark.parametrize("rows", ROWS)
def test_statistics_of_96_channels_are_those_of_three_calls_of_32(lib, rows):
    """the summation order of a column depends on the row count alone: slices computed as they are completed can be shared"""
    from bcos_hip import ops
    x = _inputs(rows, 96, seed=7 * rows)[0]
    flat, xs = _pitched(x, 1024, 8)
    whole = ops.slice_batch_stats(xs, torch.empty(96, device=DEV), torch.empty(96, device=DEV))
    mean, var = torch.full((96,), float("nan"), device=DEV), torch.full((96,), float("nan"), device=DEV)
    for lo in (64, 0, 32):
        ops.slice_batch_stats(xs[:, lo:lo + 32], mean[lo:lo + 32], var[lo:lo + 32])
    assert torch.equal(mean, whole[0]) and torch.equal(var, whole[1])
    dense = ops.slice_batch_stats(x[:, 32:64].contiguous().to(DEV), torch.empty(32, device=DEV), torch.empty(32, device=DEV))
    assert torch.equal(dense[0], whole[0][32:64]) and torch.equal(dense[1], whole[1][32:64])
    wide = ops.slice_batch_stats(_pitched(torch.cat([x, x[:, :36]], 1), 136, 4)[1], torch.empty(132, device=DEV), torch.empty(132, device=DEV))
    assert torch.equal(wide[0][:96], whole[0]) and torch.equal(wide[1][96:], whole[1][:36])


def test_column_reductions_at_the_row_count_of_a_first_dense_block(lib):
    """rows = 200704: 1024 row blocks of 196 rows -- the unrolled row loop of a lane (rpb > 128) and the four interleaved chains of the
    finish kernels (nblk > 48), which no other case reaches -- against fp64, and the 96-versus-3-x-32 equality there"""
    from bcos_hip import ops
    rows, C = 200704, 96
    assert TE.col_plan(rows) == (1024, 196)
    g = torch.Generator().manual_seed(200704)
    x = torch.randn(rows, C, generator=g) * (torch.rand(C, generator=g) * 4 + 0.05) + torch.randn(C, generator=g) * 3
    flat, xs = _pitched(x, C + 4, 4)
    before = flat.clone()
    whole = ops.slice_batch_stats(xs, torch.empty(C, device=DEV), torch.empty(C, device=DEV))
    mean, var = torch.full((C,), float("nan"), device=DEV), torch.full((C,), float("nan"), device=DEV)
    for lo in (32, 64, 0):
        ops.slice_batch_stats(xs[:, lo:lo + 32], mean[lo:lo + 32], var[lo:lo + 32])
    assert torch.equal(mean, whole[0]) and torch.equal(var, whole[1]) and _only_slice_written(flat, xs, before)
    m64, v64, bm, bv = TE.slice_batch_stats64(x)
    rm, rv = _ratio((mean.cpu().double() - m64).abs(), bm), _ratio((var.cpu().double() - v64).abs(), bv)
    assert rm <= 1.0 and rv <= 1.0, (rm, rv)
    gvec, shift = (torch.rand(C, generator=g) + 0.5), torch.randn(C, generator=g) * 0.5
    d = torch.randn(rows, C, generator=g)
    sgx, sg, _, _ = ops.slice_relu_bwd_colsums(d.to(DEV), xs, gvec.to(DEV), shift.to(DEV), want_sg=True)
    s64, g64, bs, bg, _ = TE.slice_relu_bwd_colsums64(d, x, gvec, shift)
    r1, r2 = _ratio((sgx.cpu().double() - s64).abs(), bs), _ratio((sg.cpu().double() - g64).abs(), bg)
    assert r1 <= 1.0 and r2 <= 1.0, (r1, r2)
    part = ops.slice_relu_bwd_colsums(d[:, 32:64].contiguous().to(DEV), xs[:, 32:64], gvec[32:64].to(DEV), shift[32:64].to(DEV), want_sg=True)
    assert torch.equal(part[0], sgx[32:64]) and torch.equal(part[1], sg[32:64])
    print(f"rows 200704: worst error / bound batch_stats {max(rm, rv):.3g}, relu_bwd_colsums {max(r1, r2):.3g}")


def test_bn_reader_finish(lib):
    from bcos_hip import ops
    g = torch.Generator().manual_seed(3)
    for C, eps, mom, has_w, has_rv in ((4, 1e-5, 0.1, True, True), (72, 1e-3, 1.0, False, True), (260, 1e-5, 0.0, True, True),
                                       (1000, 1e-5, 0.25, True, False)):
        var = torch.rand(C, generator=g) * 10 ** (torch.rand(C, generator=g) * 8 - 6)
        var[0] = 0.0
        w, rv = torch.randn(C, generator=g), torch.rand(C, generator=g) + 0.1
        buf = torch.full((3, C + 8), float("nan"), device=DEV)
        buf[0, 4:C + 4] = var.to(DEV)
        if has_rv:
            buf[1, 4:C + 4] = rv.to(DEV)
        run = buf[1, 4:C + 4] if has_rv else None
        rstd, gv = ops.bn_reader_finish(buf[0, 4:C + 4], w.to(DEV) if has_w else None, eps, running_var=run, momentum=mom)
        e_rstd = 1.0 / torch.sqrt(var.double() + eps)
        assert bool(((rstd.cpu().double() - e_rstd).abs() <= 2.0 ** -22 * e_rstd).all())
        e_g = e_rstd * (w.double() if has_w else 1.0)
        assert bool(((gv.cpu().double() - e_g).abs() <= 3 * 2.0 ** -23 * e_g.abs()).all())
        if has_w:
            assert bool(((gv.cpu().double() - w.double() * rstd.cpu().double()).abs() <= 2.0 ** -24 * e_g.abs() * (1 + 2.0 ** -20)).all())
        else:
            assert torch.equal(gv, rstd)
        assert _same_bits(buf[0, 4:C + 4].cpu(), var)
        if has_rv:
            e_rv = (1 - mom) * rv.double() + mom * var.double()
            assert bool(((buf[1, 4:C + 4].cpu().double() - e_rv).abs() <= 2.0 ** -22 * ((1 - mom) * rv.double() + mom * var.double()) + 2.0 ** -149).all())
        else:
            assert bool(buf[1].isnan().all())
        assert bool(buf[:, :4].isnan().all()) and bool(buf[:, C + 4:].isnan().all()) and bool(buf[2].isnan().all())


@pytest.mark.parametrize("C", CHANNELS)
def test_slice_relu_bwd_colsums(lib, C):
    from bcos_hip import ops
    worst = 0.0
    for rows in ROWS:
        x, gvec, shift, d, _, _, _ = _inputs(rows, C, seed=31 * rows + C)
        rstd = torch.rand(C, generator=torch.Generator().manual_seed(rows + C)) + 0.5
        dd, gg, rr = d.to(DEV), gvec.to(DEV), rstd.to(DEV)
        for (pitch, off), has_sh in zip(_layouts(C), (True, False, True)):
            sh = shift if has_sh else None
            flat, xs = _pitched(x, pitch, off)
            before = flat.clone()
            sgx, sg, gw, coef = ops.slice_relu_bwd_colsums(dd, xs, gg, sh.to(DEV) if has_sh else None, rstd=rr, want_sg=True, want_gw=True,
                                                           want_coef=True)
            assert _only_slice_written(flat, xs, before) and _same_bits(dd.cpu(), d), (rows, C, pitch)
            sgx, sg, gw, coef = (t.cpu() for t in (sgx, sg, gw, coef))
            s64, g64, bs, bg, gate = TE.slice_relu_bwd_colsums64(d, x, gvec, sh)
            assert torch.equal(gate, DE.slice_affine_rows32(x, gvec, sh, None, True)[0] > 0)
            r1, r2 = _ratio((sgx.double() - s64).abs(), bs), _ratio((sg.double() - g64).abs(), bg)
            worst = max(worst, r1, r2)
            assert r1 <= 1.0 and r2 <= 1.0, (rows, C, pitch, r1, r2)
            e_gw = sgx.double() * rstd.double()
            assert bool(((gw.double() - e_gw).abs() <= 2.0 ** -24 * e_gw.abs() + 2.0 ** -149).all()), (rows, C, pitch)
            e_coef = -(gvec.double() * sgx.double()) * rstd.double() ** 2 / rows
            assert bool(((coef.double() - e_coef).abs() <= 5 * 2.0 ** -24 * e_coef.abs() + 2.0 ** -149).all()), (rows, C, pitch)
            # the optional outputs change nothing of the others
            only = ops.slice_relu_bwd_colsums(dd, xs, gg, sh.to(DEV) if has_sh else None)
            assert torch.equal(only[0].cpu(), sgx) and only[1] is None and only[2] is None and only[3] is None
    print(f"bcos_slice_relu_bwd_colsums C={C}: worst error / bound {worst:.3g}")


@pytest.mark.parametrize("C", CHANNELS)
def test_slice_bn_bwd_acc(lib, C):
    from bcos_hip import ops
    worst = 0.0
    for rows in ROWS:
        x, gvec, shift, d, g_old, mean, coef = _inputs(rows, C, seed=57 * rows + C)
        dd = d.to(DEV)
        for (pitch, off), (has_sh, has_mean, acc) in zip(_layouts(C), ((True, True, True), (False, True, False), (True, False, True))):
            sh, mn = (shift if has_sh else None), (mean if has_mean else None)
            flat, xs = _pitched(x, pitch, off)
            before = flat.clone()
            gflat, gs = _pitched(g_old, pitch, off)
            if not acc:
                gflat.fill_(float("nan"))                                     # accumulate = 0 must ignore what g holds
            dev = lambda t: t.to(DEV) if t is not None else None              # noqa: E731
            ops.slice_bn_bwd_acc(dd, gs, xs, dev(gvec), dev(sh), dev(mn), dev(coef), accumulate=acc)
            assert _only_slice_written(flat, xs, before) and _same_bits(dd.cpu(), d), (rows, C, pitch)
            assert _only_slice_written(gflat, gs), (rows, C, pitch)
            want, bound, gate = TE.slice_bn_bwd_acc64(d, g_old, x, gvec, sh, mn, coef, accumulate=acc)
            r = _ratio((gs.cpu().double() - want).abs(), bound)
            worst = max(worst, r)
            assert r <= 1.0, (rows, C, pitch, r)
    print(f"bcos_slice_bn_bwd_acc C={C}: worst error / bound {worst:.3g}")


@pytest.mark.parametrize("C", CHANNELS)
def test_gates_are_the_forwards_decision_and_no_variance_term_is_the_explanation_kernel(lib, C):
    """gate of both backward kernels <=> the forward kernel's y > 0, on inputs with exact zeros and pre-activations at rounding level;
    mean / coef NULL writes the bits of bcos_slice_affine_bwd_acc"""
    from bcos_hip import ops
    rows = 257
    x, gvec, shift, d, g_old, _, _ = _inputs(rows, C, seed=900 + C)
    ones = torch.ones(rows, C, device=DEV)
    for (pitch, off), has_sh in zip(_layouts(C), (True, False, True)):
        sh = shift.to(DEV) if has_sh else None
        flat, xs = _pitched(x, pitch, off)
        y = ops.slice_affine_rows(xs, gvec.to(DEV), sh, relu=True)
        fwd = y > 0
        G = torch.full((rows, C), float("nan"), device=DEV)
        ops.slice_bn_bwd_acc(ones, G, xs, gvec.to(DEV), sh, None, None, accumulate=False)        # d = 1, g != 0: nonzero exactly where the gate is open
        assert torch.equal(G != 0, fwd), (C, pitch)
        # colsums: row by row for the rows of special values, and over all rows with integer d (exact sums in any order)
        for r in range(5):
            e = torch.zeros(rows, C, device=DEV)
            e[r] = 1.0
            sg = ops.slice_relu_bwd_colsums(e, xs, gvec.to(DEV), sh, want_sg=True)[1]
            assert torch.equal(sg != 0, fwd[r]) and torch.equal(sg, fwd[r].float()), (C, pitch, r)
        di = torch.randint(-8, 9, (rows, C), generator=torch.Generator().manual_seed(C)).float().to(DEV)
        sg = ops.slice_relu_bwd_colsums(di, xs, gvec.to(DEV), sh, want_sg=True)[1]
        assert torch.equal(sg, (di * fwd).sum(0)), (C, pitch)
        # no variance term: bit for bit the explanation-mode kernel, accumulating or not
        for acc in (False, True):
            a, b = _pitched(g_old, pitch, off), _pitched(g_old, pitch, off)
            ops.slice_bn_bwd_acc(d.to(DEV), a[1], xs, gvec.to(DEV), sh, None, None, accumulate=acc)
            ops.slice_affine_bwd_acc(d.to(DEV), b[1], x=xs, scale=gvec.to(DEV), shift=sh, relu=True, accumulate=acc)
            assert _same_bits(a[1], b[1]) and _only_slice_written(a[0], a[1]), (C, pitch, acc)


# ---- the plan ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def steps(lib):
    """ONE step through the plan, one more from the same state, and one through the per-layer path: shared by the tests below"""
    import copy
    from bcos_hip import densenet_engine
    base, x, target = TC.tiny_net(DEV)
    nets = dict(plan=copy.deepcopy(base), again=copy.deepcopy(base), layers=copy.deepcopy(base))
    for k in ("plan", "again"):
        densenet_engine.attach(nets[k])
    res = {k: TC.step(n, x, target) for k, n in nets.items()}
    return nets, res, x


def test_plan_step_against_the_reference_fixture(steps):
    nets, res, _ = steps
    assert res["plan"]["node"] == "_TrainStepFnBackward"
    TC.check_against_fixture(res["plan"], nets["plan"], "plan, MI355X")


def test_per_layer_step_against_the_reference_fixture(steps):
    nets, res, _ = steps
    assert res["layers"]["node"] != "_TrainStepFnBackward"
    TC.check_against_fixture(res["layers"], nets["layers"], "layers, MI355X")


def test_plan_against_the_per_layer_path(steps):
    nets, res, _ = steps
    TC.check_same_step(res["plan"], res["layers"], 1e-5, 1e-4, "plan vs layers")
    for (k, a), (_, b) in zip(nets["plan"].named_buffers(), nets["layers"].named_buffers()):
        if a.dtype.is_floating_point:
            assert TC.rel(a, b) <= 1e-5, k
        else:
            assert torch.equal(a, b), k


def test_running_var_follows_the_batch_as_on_the_per_layer_path(lib):
    """from buffers that are NOT the batch variance (the fixture's own are: its update is a no-op), with two norms of other momenta:
    every running_var moves, and to where the per-layer path moves it"""
    import copy
    from bcos_hip import densenet_engine
    base, x, target = TC.tiny_net(DEV)
    base.model.features[6].denselayer3.norm1.momentum = 0.5
    base.model.features[7][0].momentum = 1.0
    start = TC.scale_running_var(base)
    nets = [copy.deepcopy(base), copy.deepcopy(base)]
    densenet_engine.attach(nets[0])
    res = [TC.step(n, x, target) for n in nets]
    assert res[0]["node"] == "_TrainStepFnBackward" and res[1]["node"] != "_TrainStepFnBackward"
    assert TC.check_buffers(nets[0], nets[1], start, what="running_var, MI355X") == 23
    TC.check_same_step(res[0], res[1], 1e-5, 1e-4, "running_var, MI355X")


def test_two_steps_from_the_same_state_are_bit_equal(steps):
    _, res, _ = steps
    a, b = res["plan"], res["again"]
    assert torch.equal(a["out"], b["out"]) and torch.equal(a["gx"], b["gx"]) and a["loss"] == b["loss"]
    for n, g in a["grads"].items():
        assert torch.equal(g, b["grads"][n]), n


def test_inference_plan_behind_the_step(steps):
    """net.eval() after the step: the fused inference plan reads the updated statistics and agrees with the module path"""
    from bcos_hip import densenet_engine
    nets, _, x = steps
    net = nets["again"]
    net.eval()
    with torch.no_grad():
        fused = net(x)
        densenet_engine.detach(net)
        assert TC.rel(fused, net(x)) <= 1e-5
