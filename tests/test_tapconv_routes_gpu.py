"""`-m gpu`: every case of tests/tapconv_cases.py -- every tile launcher of bcos_tapconv_ops with every epilogue kind it can take --
launched through the C ABI and judged PER OUTPUT ELEMENT against the same operation in fp64.

For a case: the three structs are built once, the route query (bcos_tapconv_route_query) is asked and must give the launcher, loop and
epilogue kind the table expects, and the launch is issued with the same structs.  The fp64 reference is `lin64` by conv2d from the same
fp32 inputs followed by the epilogue expression documented in include/bcos_hip.h, stage by stage; with every stage goes the bound of
what it computes:

  * contraction:  |lin - lin64| <= LIN_BOUND ||a_row|| ||w_col||  (2e-6: the bound the header states for every contraction loop), times
    |col_scale row_scale| where those factors are applied;
  * plain launches: that bound carried through the expression (times |mul|, ...), plus 4 fp32 ulps of the stored value.  The row-scaled
    addend out = acc + (rowadd_scale rowadd + addend) computes the term in parentheses in fp32 before it meets the accumulator: its product
    and its sum are rounded once each, and where they cancel (or cancel against acc) those roundings are not ulps of the stored value.
    One fp32 ulp of |rowadd_scale rowadd| and one of |rowadd_scale rowadd + addend| are therefore allowed on top (twice the half-ulp
    rounding of each operation).  Without them the expression evaluated in plain fp32 from an EXACTLY rounded contraction misses the
    bound by the same factor as every launcher, the fp32-MFMA loop included (10.02 x on case cfg128_x3-b8_rowadd, both ways);
  * B-cos launches: with V >= |lin + bias| the upper bound ||a_row|| ||w_col|| |factors| + |bias| of the scaled value and n the norm,
    |y - y64| <= Y_BOUND (B / 2) V S(V),  |s - s64| <= S_BOUND (B - 1) S(V),  |n - n64| <= N_BOUND n64  with S(V) = V / n for B = 2 and
    (V / n + 1e-6)^(B - 1) in the power form -- for B = 2 without bias exactly the 4e-6 ||patch|| ||w||^2 / 3e-6 ||w|| / 5e-6 forms of
    test_patch_loop_dynamic_range_inside_an_image (y has two factors of lin: twice its relative bound).  Stages behind the scale multiply
    the bounds by |ch_scale|; those that ADD (ch_shift, addend) or evaluate a function (GELU) bring 4 fp32 ulps of the stored value, the
    roundings of their own fp32 arithmetic.  The constant-gate GELU v Phi(v) has slope <= 1.13 and its gate an absolute error <= 1.5e-7
    (csrc/bcos_internal.h: bcos_gelu_gate, Abramowitz & Stegun 7.1.26), so y's bound becomes 1.13 bound + 1.5e-7 |v| and s's
    Phi bound_s + |s| (0.4 bound_y + 1.5e-7).
  * a ReLU that gates by the sign of its own input v is continuous in `out`, and in scale_out where v has no additive stage (v -> 0 takes
    s -> 0 with it).  Behind ch_shift / addend the stored scale jumps at v = 0: an element whose |v64| is inside v's own bound may
    legitimately come out with either gate, and is held to the bound against the open OR the closed value.  No element is left out.
  * out_absmax / out2_absmax: bit-equal to the row maxima of the tensor actually written.
  * nothing else is written: NaN guard bands, the columns Cout .. out_pitch of every pixel and the pixels a strided / offset mapping
    does not address keep the NaN they were filled with.
"""
import ctypes as C
import json
import math
import os

import pytest
import torch
import torch.nn.functional as F

import tapconv_cases as tc
from tapconv_cases import LIN_BOUND, N_BOUND, S_BOUND, Y_BOUND

pytestmark = pytest.mark.gpu
DEV = "cuda"
GELU_GATE_ERR = 1.5e-7
GELU_SLOPE = 1.13

WORST = {}          # route -> {tensor: (worst error / bound, case id)}
ROWADD_BARE = {}    # rowadd case -> (worst error / bound without the ulps of the row-scaled term, worst error / bound as asserted)


@pytest.fixture(scope="module")
def blib(hip_lib):
    from bcos_hip import lib
    yield lib
    rows = {r: {k: (round(v, 4), cid) for k, (v, cid) in d.items()} for r, d in sorted(WORST.items())}
    print("\nworst error / bound per route and tensor:")
    for r, d in rows.items():
        print(f"  {r:16s} " + "  ".join(f"{k}={v[0]:.3f}" for k, v in sorted(d.items())))
    if ROWADD_BARE:
        print("row-scaled addend, worst error / bound (without | with the two ulps of the term):")
        for cid, (bare, full) in ROWADD_BARE.items():
            print(f"  {cid:32s} {bare:7.3f} | {full:.3f}")
    path = os.environ.get("BCOS_ROUTE_REPORT")
    if path:
        with open(path, "w") as f:
            json.dump(rows, f, indent=1)


def _ulp(x):
    """one fp32 unit in the last place of |x| (fp64 tensor in, fp64 out)"""
    return torch.ldexp(torch.ones_like(x), (x.float().abs().frexp().exponent - 24).to(torch.int32)).double() * (x != 0)


def reference(b, rowadd_ulps=True):
    """fp64 values and per-element bounds of every output tensor of the case, on the row grid: {name: (value, bound, alt)} with tensors
    [N, P', Q', width] (P', Q': the row grid, or the output pixels of a depth-to-space launch) and `pix` [N, P', Q'], the output pixel of
    every row."""
    case = b.case
    r, e = case.r, case.e
    G, k = b.G, r.k
    N, P, Q = r.N, r.P, r.Q
    cols = G * r.Cout
    Cg = r.C
    dev = b.a_full.device
    x = b.a_full[..., :G * Cg].double().permute(0, 3, 1, 2)
    w64 = b.w.double()
    wk = w64.view(cols, k, k, Cg).permute(0, 3, 1, 2)
    lin = F.conv2d(x, wk, stride=r.st, padding=r.pd, dilation=r.dil, groups=G).permute(0, 2, 3, 1)                 # [N, P, Q, cols]
    ones = torch.ones(G, Cg, k, k, device=dev, dtype=torch.float64)
    pn2 = F.conv2d(x * x, ones, stride=r.st, padding=r.pd, dilation=r.dil, groups=G).permute(0, 2, 3, 1).clamp_min(0)      # [N, P, Q, G]
    assert lin.shape[1:3] == (P, Q)
    wn = w64.flatten(1).norm(dim=1)                                                                                  # ||w_col|| [cols]
    grp = torch.arange(cols, device=dev) // r.Cout
    D = pn2.sqrt()[..., grp] * wn
    sumsq = pn2[..., grp]
    if r.cgroup:      # depth to space: column (dh * 2 + dw) * Gc + c of row (n, i, j) is channel c of output pixel (n, 2 i + dh, 2 j + dw)
        Gc = r.Cout // 4

        def d2s(t):
            return t.view(N, P, Q, 2, 2, Gc).permute(0, 1, 3, 2, 4, 5).reshape(N, 2 * P, 2 * Q, Gc)
        lin, D = d2s(lin), d2s(D)
        P, Q, cols = 2 * P, 2 * Q, Gc
        sh, h0 = 1, 0
    else:
        sh, h0 = b.out_sh, b.h0
    n_i = torch.arange(N, device=dev).view(N, 1, 1)
    pix = (n_i * b.OH + torch.arange(P, device=dev).view(1, P, 1) * sh + h0) * b.OW + torch.arange(Q, device=dev).view(1, 1, Q) * sh + h0
    T = b.t
    pitch = b.out_pitch

    def px(name):                      # a per-pixel side tensor at every row's pixel -> [N, P, Q, 1]
        return T[name].double().reshape(-1)[pix].unsqueeze(-1)

    def el(name, width=None):          # a tensor indexed like `out` -> [N, P, Q, width]
        return T[name].double().reshape(b.npx, pitch)[pix][..., :(width or b.out_c)]

    def ch(name):
        return T[name].double()

    f = torch.ones(cols, device=dev, dtype=torch.float64)
    if e.col_scale:
        f = f * ch("col_scale")
    if e.flags & tc.EPI_UNIT_NORM_W:
        f = f / wn
    f = f.view(1, 1, 1, cols)
    if e.row_scale:
        f = f * px("row_scale")
    v = lin * f
    err = LIN_BOUND * D * f.abs()
    V = D * f.abs()
    if e.bias:
        v = v + ch("bias")
        V = V + ch("bias").abs()
    out = {}
    arg = None
    if e.max_out > 1:
        M = e.max_out
        vu = v.reshape(N, P, Q, cols // M, M)
        v, arg = vu.max(dim=-1)
        err = err.reshape(N, P, Q, cols // M, M).amax(-1)
        V = V.reshape(N, P, Q, cols // M, M).amax(-1)
        sumsq = sumsq[..., ::M]
    s = torch.ones_like(v)
    b_s = torch.zeros_like(v)
    post = False
    if e.norm:
        if e.a_sumsq:
            sumsq = px("a_sumsq").expand_as(v)
        n64 = (sumsq + 1e-6).sqrt() if e.bcos_mode == 1 else sumsq.sqrt() + 1e-12
        if "norm_out" in T:
            nn_ = n64[..., ::r.Cout] if G > 1 else n64[..., :1]            # one patch norm per pixel and group
            out["norm_out"] = (nn_, N_BOUND * nn_, None)
        fast = e.b == 2.0 and not (e.flags & tc.EPI_FORCE_POW)
        bm1 = e.b - 1.0
        if fast:
            s, S_up = v.abs() / n64, V / n64
        else:
            s, S_up = (v.abs() / n64 + 1e-6) ** bm1, (V / n64 + 1e-6) ** bm1
        b_s = S_BOUND * bm1 * S_up
        err = Y_BOUND * (e.b / 2.0) * V * S_up
        v = v * s
    if e.ch_scale:
        cs = ch("ch_scale")[:cols].view(1, 1, 1, -1)
        v, s, err, b_s = v * cs, s * cs, err * cs.abs(), b_s * cs.abs()
    if e.ch_shift:
        v = v + ch("ch_shift")[:cols]
        post = True
    shifted = e.ch_shift or e.addend
    assert e.addend or not e.rowadd          # (the table's row-scaled addend comes with an addend)
    if e.addend:
        if e.addend_sub > 1:
            sb = e.addend_sub
            ohh, oww = (b.OH + sb - 1) // sb, (b.OW + sb - 1) // sb
            hh, ww = (pix // b.OW) % b.OH, pix % b.OW
            on = (hh % sb == 0) & (ww % sb == 0)
            api = (n_i * ohh + hh // sb) * oww + ww // sb
            ad = T["addend"].double().reshape(-1, pitch)[api * on][..., :cols] * on.unsqueeze(-1)
        else:
            ad = el("addend")
        if e.rowadd:
            prod = px("rowadd_scale") * el("rowadd")
            ad = ad + prod
            if rowadd_ulps:
                err = err + _ulp(prod) + _ulp(ad)          # the two fp32 roundings of the term in parentheses (module docstring)
        v = v + ad
        post = True
    s_alt = None
    if e.relu == 2:
        gate = 0.5 * (1.0 + torch.erf(v / math.sqrt(2.0)))
        b_s = b_s * gate + s.abs() * (0.4 * err + GELU_GATE_ERR)
        err = GELU_SLOPE * err + v.abs() * GELU_GATE_ERR
        s, v = s * gate, v * gate
        post = True
    elif e.relu == 1:
        if e.relu_gate:
            open_ = el("relu_gate") > 0
        else:
            open_ = v > 0
            if e.norm and shifted:           # the stored scale jumps where v crosses zero: either gate is right inside v's own bound
                near = v.abs() <= err + 4 * _ulp(v)
                s_alt = torch.where(near, torch.where(open_, torch.zeros_like(s), s), torch.full_like(s, float("nan")))
        s = torch.where(open_, s, torch.zeros_like(s))
        v = torch.where(open_, v, torch.zeros_like(v))
    ulps = 4 if (post or not e.norm) else 0
    if "scale_out" in T:
        sv, sb_, sa = s, b_s + (ulps * _ulp(s) if e.norm else 0), s_alt
        if arg is not None:      # MaxOut: the scale at the winning filter of every unit, zero at the others
            hot = F.one_hot(arg, e.max_out).double()
            sv = (hot * s.unsqueeze(-1)).reshape(N, P, Q, -1)
            sb_ = (hot * sb_.unsqueeze(-1)).reshape(N, P, Q, -1)
        out["scale_out"] = (sv, sb_, sa)
    o1, b1 = v, err
    if e.mul:
        if e.flags & tc.EPI_MUL_FROM_ACT:
            a_ = el("mul")
            den = ch("mul_csc").abs() * px("mul_norm")
            m = torch.where(a_ > 0, ch("mul_csc") * ((a_ - ch("mul_csh")).abs() / den).sqrt(), torch.zeros_like(a_))
        else:
            m = el("mul")
        o1, b1 = v * m, err * m.abs()
    out["out"] = (o1, b1 + ulps * _ulp(o1), None)
    if e.out2:
        o2, b2 = v, err
        if e.mul2:
            o2, b2 = o2 * el("mul2"), b2 * el("mul2").abs()
        if e.gate2:
            g2 = (el("gate2") > 0).double()
            o2, b2 = o2 * g2, b2 * g2
        out["out2"] = (o2, b2 + ulps * _ulp(o2), None)
    return out, pix


def judge(b, name, val, bound, alt, pix):
    """worst |result - fp64| / bound over EVERY addressed element of tensor `name`; everything else must still be NaN"""
    buf, extra = b.guards[name]
    assert torch.isnan(buf[:extra]).all() and torch.isnan(buf[-extra:]).all(), (b.case.id, name, "write outside the tensor")
    res = b.t[name].double().reshape(b.npx, -1)
    width = val.shape[-1]
    full = torch.full_like(res, float("nan"))
    fb = torch.zeros_like(res)
    flat = pix.reshape(-1)
    full[flat, :width] = val.reshape(-1, width)
    fb[flat, :width] = bound.reshape(-1, width)
    addressed = ~torch.isnan(full)
    assert torch.isnan(res[~addressed]).all(), (b.case.id, name, "an element outside the launch's output mapping was written")
    assert torch.isfinite(res[addressed]).all(), (b.case.id, name, "an addressed element was not written, or is not finite")
    d = (res - full).abs()
    if alt is not None:
        fa = torch.full_like(res, float("nan"))
        fa[flat, :width] = alt.reshape(-1, width)
        d = torch.where(torch.isnan(fa), d, torch.minimum(d, (res - fa).abs()))
    ratio = d[addressed] / (fb[addressed] + 1e-300)
    ratio = torch.where(d[addressed] == 0, torch.zeros_like(ratio), ratio)
    return ratio.max().item()


def run_case(blib, case):
    lib = blib.load()
    b = tc.Built(case, DEV, blib)
    torch.cuda.synchronize()
    with tc.with_options(blib, b.options()):
        q = blib.route_query(b.ops, b.geom, b.epi)
        r = case.r
        assert (q["route"], q["loop"], q["epi_kind"], q["norm"], q["chunks"], q["ch_pass"]) == \
               (r.route, r.loop, case.kind, int(case.e.norm), r.chunks, r.ch_pass), (case.id, q)
        blib.check(lib.bcos_tapconv_ops(C.byref(b.ops), C.byref(b.geom), C.byref(b.epi), None), "bcos_tapconv_ops")
        torch.cuda.synchronize()
    exp, pix = reference(b)
    ratios = {}
    for name, (val, bound, alt) in exp.items():
        ratios[name] = judge(b, name, val, bound, alt, pix)
    for am, src in (("out_absmax", "out"), ("out2_absmax", "out2")):
        if am in b.t:
            written = b.t[src].reshape(b.npx, -1)
            want = torch.nan_to_num(written, nan=0.0).abs().amax(dim=1).view(torch.int32)
            assert torch.equal(b.t[am], want), (case.id, am)
    if case.e.rowadd:          # for the record: the same result against the bound WITHOUT the two ulps of the row-scaled term (not asserted)
        val, bound, alt = reference(b, rowadd_ulps=False)[0]["out"]
        ROWADD_BARE[case.id] = (judge(b, "out", val, bound, alt, pix), ratios["out"])
    return ratios


@pytest.mark.parametrize("case", tc.CASES, ids=lambda c: c.id)
def test_case_against_fp64_per_element(blib, case):
    ratios = run_case(blib, case)
    print(case.id, case.r.route, {k: f"{v:.3f}" for k, v in ratios.items()})
    slot = WORST.setdefault(case.r.route, {})
    for k, v in ratios.items():
        if k not in slot or v > slot[k][0]:
            slot[k] = (v, case.id)
    bad = {k: v for k, v in ratios.items() if not v <= 1.0}
    assert not bad, (case.id, "worst error / bound", ratios)


def test_production_launches_take_routes_the_table_covers(blib, monkeypatch):
    """Every bcos_tapconv_ops launch the Python layer issues for the BASELINE configurations -- forward + explanation of ResNet-50 at batch
    256, ViT-Ti at batch 512, CLIP RN50 at batch 256, and one ResNet-50 training step at batch 64 through the plans (synthetic weights) --
    is asked for its route first; every (route, direction, epilogue kind, loop) they use must be one the case table holds to fp64, and
    every workload must have recorded launches."""
    from bcos_hip import engine, synth, vit_engine
    lib = blib.load()
    launch = lib.bcos_tapconv_ops
    used = {}
    where = ["?"]

    def recorder(o, g, e, stream):
        r = blib.TapconvRoute()
        rc = lib.bcos_tapconv_route_query(o, g, e, C.byref(r))
        if rc == 0:
            key = (lib.bcos_tapconv_route_name(r.route).decode(), r.norm, r.epi_kind, blib.LOOP_NAMES[r.loop])
            used.setdefault(key, {}).setdefault(where[0], 0)
            used[key][where[0]] += 1
        return launch(o, g, e, stream)

    monkeypatch.setattr(lib, "bcos_tapconv_ops", recorder)
    covered = {(c.r.route, int(c.e.norm), c.kind, c.r.loop) for c in tc.CASES}

    def prepared(net, n):
        x = synth.synthetic_images(n).to(DEV)
        with torch.no_grad():
            synth.calibrate(net, x[:8])
        return x

    where[0] = "resnet50 b256 explain"
    net = synth.build_bcosified_resnet("resnet50").to(DEV)
    x = prepared(net, 256)
    out = engine.attach(net).explain(x)
    assert torch.isfinite(out["dynamic_linear_weights"]).all()
    where[0] = "resnet50 b64 training step"
    net.train()
    target = F.one_hot(torch.arange(64) % 1000, 1000).float().to(DEV)
    F.binary_cross_entropy_with_logits(net(x[:64]), target).backward()
    assert getattr(net._bcos_engine, "_train_plan", None) is not None, "the training step did not go through the training plan"
    assert all(torch.isfinite(p.grad).all() for p in net.parameters() if p.grad is not None)
    del net, out
    where[0] = "vit-ti b512 explain"
    vit = synth.build_bcosified_vit("simple_vit_ti_patch16_224").to(DEV)
    x = prepared(vit, 512)
    out = vit_engine.attach(vit).explain(x)
    assert torch.isfinite(out["dynamic_linear_weights"]).all()
    del vit, out
    where[0] = "clip rn50 b256 explain"
    clip = synth.build_bcosified_clip_rn50().to(DEV)
    x = prepared(clip, 256)
    eng = engine.attach(clip)
    emb = eng.forward(x)
    out = eng.explain(x, targets=torch.full((256,), 7))
    assert torch.isfinite(emb).all() and torch.isfinite(out["dynamic_linear_weights"]).all()
    torch.cuda.synchronize()
    print("\n(route, direction, epilogue kind, loop) of the production launches, with launch counts per workload:")
    for key, cnt in sorted(used.items()):
        print(f"  {key[0]:16s} {'B-cos' if key[1] else 'plain'} kind {key[2]}  {key[3]:16s} {cnt}{'' if key in covered else '   <-- NOT IN THE CASE TABLE'}")
    labels = {w for cnt in used.values() for w in cnt}
    want = {"resnet50 b256 explain", "resnet50 b64 training step", "vit-ti b512 explain", "clip rn50 b256 explain"}
    assert labels == want, f"workloads that recorded no launch: {want - labels}"
    missing = sorted(k for k in used if k not in covered)
    assert not missing, f"production launches on (route, direction, epilogue kind, loop) no case covers: {missing}"
