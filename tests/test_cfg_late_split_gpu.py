"""The late guidance split of forward_cfg (unet.py::forward_ndhwc / cs_unet.hip::forward): in F16X3 math the first
context-dependent block (input_blocks.4 = [ResBlock, SpatialTransformer]) runs its ResBlock and its transformer block up to the
attn1.to_out product ONCE, at batch B, and the guidance halves part where attn2's row vector is added
(cs_twin_layernorm_pair16).  Against the block-granular split (CsDebug.no_cfg_late_split = 1: duplicate at the block's entry)
and against the duplicated batch it must give the same bits, on both drivers; the GEMM records prove that the shared launches
really ran at B S rows; fp32 math does not take the route."""
import pytest
import torch

pytestmark = pytest.mark.gpu

B = 2
S4 = 16 * 8 * 8          # voxels per sample at input_blocks.4 (dims = 3: H, W halved once)


def _models(cfg, math, native=True):
    from commonscenes_amd import synth
    from commonscenes_amd.unet import DiffusionUNet, unet_param_shapes
    from commonscenes_amd.unet_native import NativeDiffusionUNet
    sd = synth.synth_state_dict(unet_param_shapes(cfg), device="cuda")
    py = DiffusionUNet(cfg, conditioning_key="crossattn", device="cuda").set_math(math)
    py.load_state_dict(sd)
    nat = None
    if native:
        nat = NativeDiffusionUNet(cfg, conditioning_key="crossattn", device="cuda", math=math)
        nat.load_state_dict(sd)
    return py, nat


def _inputs(nb, tag):
    from commonscenes_amd import synth
    x = synth.gaussian_like(f"{tag}:x", (nb, 3, 16, 16, 16)).cuda()
    t = torch.tensor([981, 37, 501][:nb], dtype=torch.long).cuda()          # a different t per sample
    c_in = synth.gaussian_like(f"{tag}:c", (2 * nb, 1, 1280)).cuda()         # [uc; c]
    return x, t, c_in


_REDUCED = {}


def _reduced():
    """the reduced-width models, inputs and the three evaluations per driver, computed once"""
    if _REDUCED:
        return _REDUCED
    from commonscenes_amd import configs as K, lib as L, ops
    py, nat = _models(K.reduced(K.UNET_CROSSATTN), "f16x3")
    x, t, c_in = _inputs(B, "late")
    ops.clear_status()
    for name, df in (("py", py), ("nat", nat)):
        late = df.forward_cfg(x, t, c_in)
        with L.debug_override(no_cfg_late_split=1):
            block = df.forward_cfg(x, t, c_in)
        dup = df(torch.cat([x, x]), torch.cat([t, t]), c_crossattn=[c_in])
        torch.cuda.synchronize()
        _REDUCED[name] = (late, block, dup)
    _REDUCED["status"] = ops.read_status()
    _REDUCED["models"] = (py, nat, x, t, c_in)
    return _REDUCED


@pytest.mark.parametrize("driver", ["py", "nat"])
def test_late_split_equals_block_granular_split_and_duplicated_batch(driver):
    r = _reduced()
    late, block, dup = r[driver]
    assert late.shape == (2 * B, 3, 16, 16, 16) and torch.isfinite(late).all() and r["status"] == 0
    assert torch.equal(late, block), "late split != block-granular split"
    assert torch.equal(late, dup), "forward_cfg != forward on the duplicated batch"
    assert not torch.equal(late[:B], late[B:]), "the guidance halves got the same context"


def test_native_driver_equals_python_driver_on_the_late_route():
    r = _reduced()
    assert torch.equal(r["py"][0], r["nat"][0])


def _rows(rec):
    """output rows of a GEMM record (a Winograd-W record carries its position launch's rows: npos per `variant` outputs)"""
    return rec["m"] // rec["npos"] * (rec["npos"] - 2) if rec.get("wino") else rec["m"]


def test_shared_launches_run_at_half_the_rows():
    """ops.GEMM_PROFILE of one forward_cfg per route: the same launches in the same order, and exactly input_blocks.4's two
    convs, its skip conv, proj_in, q|k|v and attn1.to_out differ -- B S rows on the late route, 2 B S on the block-granular"""
    from commonscenes_amd import lib as L, ops
    py, _, x, t, c_in = _reduced()["models"]
    recs = {}
    for route in (0, 1):
        with L.debug_override(no_cfg_late_split=route):
            ops.GEMM_PROFILE = []
            try:
                py.forward_cfg(x, t, c_in)
                torch.cuda.synchronize()
                # (k as the direct form's: a Winograd-W record carries its 3 x 3 x 1 position GEMM's)
                recs[route] = [(r["n"], r["k"] * (3 if r.get("wino") else 1), _rows(r)) for r in ops.GEMM_PROFILE]
            finally:
                ops.GEMM_PROFILE = None
    late, block = recs[0], recs[1]
    assert len(late) == len(block) and [r[:2] for r in late] == [r[:2] for r in block]
    diff = [(a, b) for a, b in zip(late, block) if a[2] != b[2]]
    c_in4, c4 = 32, 64                                   # input_blocks.4 at the reduced width: ResBlock 32 -> 64
    want = {(c4, c_in4 * 27), (c4, c4 * 27), (c4, c_in4), (c4, c4), (3 * c4, c4)}      # conv1, conv2, skip, proj_in / to_out, q|k|v
    assert {a[:2] for a, _ in diff} == want, diff
    assert len(diff) == 6, diff                          # (proj_in and to_out share a shape)
    for a, b in diff:
        assert a[2] == B * S4 and b[2] == 2 * B * S4, (a, b)


def test_fp32_math_keeps_the_block_granular_split():
    from commonscenes_amd import configs as K, lib as L, ops
    py, nat = _models(K.reduced(K.UNET_CROSSATTN), "fp32")
    x, t, c_in = _inputs(B, "late32")
    for df in (py, nat):
        a = df.forward_cfg(x, t, c_in)
        with L.debug_override(no_cfg_late_split=1):
            b = df.forward_cfg(x, t, c_in)
        torch.cuda.synchronize()
        assert torch.isfinite(a).all() and torch.equal(a, b)
    ops.GEMM_PROFILE = []
    try:
        py.forward_cfg(x, t, c_in)
        torch.cuda.synchronize()
        rows = [r["m"] for r in ops.GEMM_PROFILE if (r["n"], r["k"]) == (64, 32)]      # input_blocks.4's skip conv
    finally:
        ops.GEMM_PROFILE = None
    assert rows and rows[0] == 2 * B * S4


def test_shipped_width_one_object_late_equals_block_granular():
    """shipped width, B = 1: the shared launches run 1024 rows where the duplicated batch runs 2048 -- launch rules that follow
    the batch (Winograd-W F(2,3) below 2048 rows, F(4,3) from there; the K-slice counts) are taken from the duplicated batch
    (cs_conv_plan_copies), so the bits stay"""
    from commonscenes_amd import configs as K, lib as L
    py, _ = _models(dict(K.UNET_CROSSATTN), "f16x3", native=False)
    x, t, c_in = _inputs(1, "late1")
    a = py.forward_cfg(x, t, c_in)
    with L.debug_override(no_cfg_late_split=1):
        b = py.forward_cfg(x, t, c_in)
    torch.cuda.synchronize()
    assert torch.isfinite(a).all() and torch.equal(a, b)
