"""What the backward GEMMs of gemm_bwd.hip compute, one launch at a time.  `-m gpu`.

Every case goes through `native.op_gemm_bwd` -> `l2s_op_gemm_bwd` -> launch_gemm_bwd / launch_gemm_bwd_splitk / launch_gemm_bwd_dw_dx - the product's vec
rule, slice clipping and refusals - once with f32 and once with bf16 operands, and the record the call reports back says which of the twelve kernel
instances (gemm_bwd_kernel<DX|DW, BF16, VEC>, gemm_bwd_pair_kernel<BF16, VEC>) ran.

(a) replay: the launch recorder is armed around one training step at the golden clips' shape (B = 2, T = 29, S = 9, 96 x 96), one encoder forward /
    backward at (1, 5, 88) - and the same backward with the 1x1 convs' weights frozen - and one train_refresh_weights; every distinct recorded launch
    is run again at its own size, strides, pointer alignment and slice count on integer operands.  If a call site changes, the test follows it.
(b) the edge table of tests/gemm_bwd_common.py: sizes the small step does not produce.
In (a) and (b) the whole output buffer - result, pad columns, rows past M, untouched frames of the c_T form, guards - must equal the fp64 reference
placed into the pre-fill BIT FOR BIT: integer operands under lim^2 * K * |alpha| + max|C0| < 2^24 make fp32 accumulation exact in any order, in the
f32 and in the bf16 form alike.
(c) random data on six rows of (b): the f32 form within 2e-5 * max(1, max|ref|) of the fp64 product (the bound of test_conv1d_backward_gemms); the bf16
    form, against the fp64 product of the bf16-rounded operands, within four times the error an fp32 torch product of the same rounded operands makes
    on this device plus 2^-22 * max|ref| (the two differ in summation order only).  Measured errors: profiles/gemm_bwd_op_errors.txt."""
import os

import pytest
import torch

import gemm_bwd_common as gb
from lip2speech_amd import native

pytestmark = pytest.mark.gpu

TABLE = gb.edge_table()
REFUSALS = gb.refusal_table()
_cache = {}


def prepared(key, L, seed):
    """host buffers and the fp64 reference of every half of a launch: built once, shared by the f32 and the bf16 run, never written to"""
    if key not in _cache:
        halves = gb.build(L, seed)
        for H in halves:
            H["want"] = gb.expected(H, gb.reference(H["d"], H["a"], H["b"]))
        _cache[key] = halves
    return _cache[key]


def run(L, halves, bf16, refused=None):
    """one launch on device copies of the buffers -> (the record reported back, the output buffer of every half on the host)"""
    dev = []
    for H in halves:
        D = dict(A=dev[0]["A"] if H.get("shared_A") else H["A"].cuda(), B=H["B"].cuda(), C=H["C"].cuda())
        assert all(D[k].data_ptr() % 16 == 0 for k in "ABC")
        D["ptr"] = tuple(D[k].data_ptr() + 4 * H["lay"][k.lower()][0] for k in "ABC")
        dev.append(D)
    d = L["d"]
    used = gb.used_splits(L)
    partials = torch.full((used * d["M"] * d["N"] + gb.GUARD,), gb.SENTINEL, device="cuda") if L["entry"] else None
    pair = (native.gemm_bwd_desc(**L["d2"]),) + dev[1]["ptr"] if L["pair"] else None
    rec = native.op_gemm_bwd(native.gemm_bwd_desc(**d), *dev[0]["ptr"], splits=L["splits_asked"] if L["entry"] else 0, partials=partials, bf16=bf16, pair=pair,
                             refused=refused)
    torch.cuda.synchronize()
    if partials is not None:
        assert bool((partials[used * d["M"] * d["N"]:] == gb.SENTINEL).all()), "a slice wrote past the partial matrices"
    return rec, [D["C"].cpu() for D in dev]


def mismatch(L, halves, outs):
    """None, or where the output buffers differ from the expected ones"""
    msgs = []
    for h, (H, got) in enumerate(zip(halves, outs)):
        want = H["want"].float()
        if torch.equal(got, want) and torch.equal(want.double(), H["want"]):
            continue
        bad = (got != want).nonzero().reshape(-1)
        inside = torch.zeros(got.numel(), dtype=torch.bool)
        inside[H["lay"]["c"][1].reshape(-1)] = True
        i = int(bad[0])
        msgs.append(f"half {h}: {int(inside[bad].sum())} wrong result elements, {int((~inside[bad]).sum())} changed elements outside the result; first at buffer index "
                    f"{i} (result starts at {H['lay']['c'][0]}): got {float(got[i])}, want {float(want[i])}")
    return "; ".join(msgs) or None


def check_exact(L, key, seed, bf16):
    assert gb.exactness_margin(L) < 2 ** 24
    halves = prepared(key, L, seed)
    rec, outs = run(L, halves, bf16)
    assert (rec["entry"], rec["pair"], rec["bf16"], rec["splits"], rec["vec"]) == (L["entry"], L["pair"], int(bf16), gb.used_splits(L), gb.expected_vec(L)), rec
    return rec, mismatch(L, halves, outs)


# ------------------------------------------------------------------------------------------------ (b)
@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("L", TABLE, ids=[L["name"] for L in TABLE])
def test_edge_table(L, bf16):
    rec, bad = check_exact(L, ("table", L["name"]), 1000 + TABLE.index(L), bf16)
    assert bad is None, f"{L['name']} ({'bf16' if bf16 else 'f32'}, vec {rec['vec']}, {rec['splits']} slices): {bad}"


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("L,rule", REFUSALS, ids=[r[0]["name"] for r in REFUSALS])
def test_refused_launches_write_nothing(L, rule, bf16):
    halves = gb.build(L, 7)
    refused = []
    rec, outs = run(L, halves, bf16, refused=refused)
    assert len(refused) == 1 and rule in refused[0], refused
    assert rec["name"] == "" and rec["splits"] == 0
    for H, got in zip(halves, outs):
        assert torch.equal(got, H["C"])


# ------------------------------------------------------------------------------------------------ (a)
@pytest.fixture(scope="module")
def recorded(synth_sd):
    """the distinct backward-GEMM launches of one training step, one small encoder pass and one weight refresh, in launch order"""
    import parity_common as pc
    from lip2speech_amd import synth, training
    B, T, S = 2, 29, 9
    nm = pc.fresh_native_model(synth_sd, diag=True, refresh_map=1)
    bound = {k: v.clone().cuda() for k, v in synth_sd.items() if k.startswith(("encoder.", "decoder.")) and v.is_floating_point()}
    is_buf = lambda k: k.endswith(("running_mean", "running_var", "pos_table"))      # noqa: E731
    grads = {k: torch.zeros_like(v) for k, v in bound.items() if not is_buf(k)}
    nm.train_bind(bound, grads)
    video, emb = synth.synth_video(B, T, tag="bwdrec").cuda(), synth.synth_speaker_embedding(B, tag="bwdrec").cuda()
    gum, mels = synth.synth_gumbel(B * 4, tag="bwdrec").cuda(), synth.synth_mels(B, S, tag="bwdrec").cuda()
    gate = torch.zeros(B, S, device="cuda")
    gate[:, -1] = 1
    small = synth.synth_video(1, 5, H=88, W=88, tag="bwdrec88").cuda()
    pointwise = ("banch2.0.weight", "banch2.5.weight", "banch1.2.weight", "trunk.1.0.weight")
    native.gemm_bwd_recorder_arm()
    try:
        training.model_forward_backward(nm, video, emb, gum, mels, gate)
        _, _, tape = nm.train_encoder_fwd(small)
        nm.train_encoder_bwd(small, torch.ones(1, 5, 1024, device="cuda"), tape)
        nm.train_refresh_weights()
        # the same small pass with the 1x1 convs' weights frozen (no gradient slot): their input gradients then leave the dW + dX pair and run alone -
        # the model's only stand-alone launches on 58 channels (gemm_bwd_kernel<DX, *, false>)
        nm.train_bind(bound, {k: g for k, g in grads.items() if not (k.startswith("encoder.") and k.endswith(pointwise))})
        nm.train_encoder_bwd(small, torch.ones(1, 5, 1024, device="cuda"), tape)
        torch.cuda.synchronize()
    finally:
        records = native.gemm_bwd_recorder_read(disarm=True)
    distinct, names = {}, {}
    for R in records:
        k = gb.dedup_key(R)
        distinct.setdefault(k, R)
        names.setdefault(k, set()).add(R["name"])
    return dict(total=len(records), launches=[dict(R, name="+".join(sorted(names[k]))) for k, R in distinct.items()])


def test_recorded_launches_cover_the_model_forms(recorded):
    Rs = recorded["launches"]
    print(f"\nrecorded {recorded['total']} backward-GEMM launches, {len(Rs)} distinct")
    assert Rs and all(R["bf16"] == 0 for R in Rs)
    have = lambda f: any(f(R, R["d"]) for R in Rs)      # noqa: E731
    assert have(lambda R, d: R["entry"] == 1 and R["splits"] > 1 and d["mode"] == gb.DX and d["accumulate"]), "no split-K DX with accumulate"
    assert have(lambda R, d: d["mode"] == gb.DX and d["c_T"] > 0), "no c_T DX"
    assert have(lambda R, d: R["pair"] and R["vec"] == 0), "no pair with vec = 0"
    assert have(lambda R, d: R["pair"] and R["splits"] > 1), "no pair with more than one slice"
    assert have(lambda R, d: d["mode"] == gb.DW and d["stride"] == d["taps"] > 1), "no DW with stride == taps > 1"
    assert have(lambda R, d: d["ldb"] != d["taps"] * d["Cin"]), "no launch with ldb != taps * Cin"
    assert have(lambda R, d: R["pair"] and d["K"] == 58 * 24 * 24 and d["M"] == 58), "the 33 408-row reductions of the 58-channel layers are missing"
    for R in Rs:                                          # what the recorder wrote is what the rules of the launch functions give for the descriptor
        L = gb.from_record(R)
        assert (R["splits"], R["vec"]) == (gb.used_splits(L), gb.expected_vec(L)), R


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
def test_replay_of_every_recorded_launch(recorded, bf16):
    """bit equality and untouched surroundings for every distinct launch the model made.  The replays reach both VEC forms of the DX kernel and of the
    pair kernel and the VEC form of the DW kernel: every stand-alone weight gradient of the model has dimensions in multiples of 4 on 16-byte aligned
    operands (the 58-channel layers take the pair), so gemm_bwd_kernel<DW, *, false> is launched by no call site - the edge table runs it, and the two
    together reach all twelve instances"""
    failures, reached = [], set()
    for i, R in enumerate(recorded["launches"]):
        L = gb.from_record(R)
        while gb.exactness_margin(L) >= 2 ** 24:          # a reduction too long for [-8, 8]: a narrower range, never a case dropped
            L["lim"] //= 2
            assert L["lim"] >= 1, R
        rec, bad = check_exact(L, ("replay", i), 5000 + i, bf16)
        assert (rec["splits"], rec["vec"]) == (R["splits"], R["vec"]), (rec, R)
        reached.add(gb.instance(L, bf16))
        if bad:
            d = L["d"]
            failures.append(f"{R['name']} (mode {d['mode']}, M N K {d['M']} {d['N']} {d['K']}, taps {d['taps']}, entry {R['entry']}, {R['splits']} slices, vec {R['vec']}): {bad}")
    print(f"\nreplayed {len(recorded['launches'])} distinct launches ({'bf16' if bf16 else 'f32'}); instances: {sorted(reached)}")
    assert not failures, "\n".join(failures)
    assert reached >= {t for t in gb.ALL_INSTANCES if t[2] == int(bf16) and t[:2] != ("dw", 0)}, sorted(reached)
    assert reached | {gb.instance(L, bf16) for L in TABLE} == {t for t in gb.ALL_INSTANCES if t[2] == int(bf16)}


# ------------------------------------------------------------------------------------------------ (c)
def _rounded(t):
    return t.bfloat16().float()


def _torch_fp32(d, a, b):
    """the same gradient by torch in fp32 on the device (another summation order), without alpha"""
    B, Tx, Tz, Cin, Nout, taps, stride, pad = gb.geometry(d)
    if taps == 1:
        return a @ b if d["mode"] == gb.DX else a.t() @ b
    F = torch.nn.functional
    dz = a.reshape(B, Tz, Nout).permute(0, 2, 1)
    if d["mode"] == gb.DX:
        w = b.reshape(Nout, taps, Cin).permute(0, 2, 1).contiguous()
        x = torch.zeros(B, Cin, Tx, device=a.device, requires_grad=True)
        (g,) = torch.autograd.grad(F.conv1d(x, w, padding=pad), x, dz)
        return g.permute(0, 2, 1).reshape(B * Tx, Cin)
    x = b.reshape(B, Tx, Cin).permute(0, 2, 1).contiguous()
    w = torch.zeros(Nout, Cin, taps, device=a.device, requires_grad=True)
    (g,) = torch.autograd.grad(F.conv1d(x, w, stride=stride, padding=pad), w, dz)
    return g.permute(0, 2, 1).reshape(Nout, taps * Cin)


@pytest.mark.parametrize("name", gb.RANDOM_CASES)
def test_random_data(name):
    """normal operands, unit-scale results (max|ref| 3.2 - 5.3).  Measured on the MI355X (profiles/gemm_bwd_op_errors.txt has every case): the f32 form's
    largest error 1.96e-6 (dW of pair58_k33409_s256; bound 6.9e-5); the bf16 form's largest error 1.71e-6 on the same case, where the fp32 torch
    product of the same rounded operands is off by 7.4e-6 (bound 3.0e-5); elsewhere the bf16 form is within 2.4e-7 - 6.4e-7 of the fp64 product of the
    rounded operands, torch's fp32 product within 2.2e-7 - 7.5e-7, the bounds 1.8e-6 - 4.2e-6"""
    L = next(x for x in TABLE if x["name"] == name)
    halves = gb.build(L, 9000 + gb.RANDOM_CASES.index(name), random_data=True)
    lines = []
    for bf16 in (False, True):
        rec, outs = run(L, halves, bf16)
        assert rec["bf16"] == int(bf16) and rec["vec"] == gb.expected_vec(L)
        for h, (H, got) in enumerate(zip(halves, outs)):
            d, idx = H["d"], H["lay"]["c"][1]
            a, b = (_rounded(H["a"]), _rounded(H["b"])) if bf16 else (H["a"], H["b"])
            ref = gb.reference(d, a, b)
            c0 = H["C"].double()[idx] if d["accumulate"] else 0.0
            err = float((got.double()[idx] - (c0 + d["alpha"] * ref)).abs().max())
            scale = float(ref.abs().max())
            outside = torch.ones(got.numel(), dtype=torch.bool)
            outside[idx.reshape(-1)] = False
            assert torch.equal(got[outside], H["C"][outside]), f"{name} half {h}: elements outside the result changed"
            if bf16:
                base = float((_torch_fp32(d, a.cuda(), b.cuda()).double().cpu() - ref).abs().max())
                bound = 4 * base + 2.0 ** -22 * scale
                lines.append(f"{name} half {h} bf16: kernel error {err:.3e}  fp32 torch error {base:.3e}  bound {bound:.3e}  max|ref| {scale:.3e}")
            else:
                bound = 2e-5 * max(1.0, scale)
                lines.append(f"{name} half {h} f32: kernel error {err:.3e}  bound {bound:.3e}  max|ref| {scale:.3e}")
            print(lines[-1])
            H.setdefault("checks", []).append((err, bound, lines[-1]))
    path = os.environ.get("L2S_GEMM_BWD_ERRORS")          # a run that refreshes profiles/gemm_bwd_op_errors.txt names the file to append to
    if path:
        with open(path, "a") as f:
            f.write("\n".join(lines) + "\n")
    for H in halves:
        for err, bound, line in H["checks"]:
            assert err <= bound, line
