"""CPU: the stage-1 pose flow's definition (tests/flow_ref.py), its synthetic weights, the checkpoint loader's rules and the argument checks of
the C-ABI entries of csrc/flow.hip.  No GPU."""
import ctypes as C

import numpy as np
import pytest
import torch

from egohmr_amd import synthetic as syn
from tests import flow_ref as fr
from tests.test_stage1_cpu import FLAGS

ALL_OFF = dict(with_focal_length=False, with_bbox_info=False, with_cam_center=False)


@pytest.fixture(scope="module")
def flow_sd():
    return syn.make_stage1_flow_state_dict(0)


@pytest.fixture(scope="module")
def flow_sd_bn():
    return syn.make_stage1_flow_state_dict(1, batch_norm=True, **ALL_OFF)


@pytest.fixture(scope="module")
def full_sd(flow_sd):
    return {**syn.make_stage1_state_dict(0), **flow_sd}


def _rows(sd, R=6, seed=0):
    g = np.random.Generator(np.random.PCG64(900 + seed))
    ctx = fr.transform_keys(sd)[2]["transform_net.blocks.0.context_layer.weight"].shape[1]
    c = np.concatenate([g.normal(scale=0.3, size=(R, ctx - 2560)), g.uniform(0, 2, size=(R, 2048)), g.normal(size=(R, 512))], 1)
    z = g.normal(size=(R, 144))
    z[0] = 0.0                                                       # the mode
    return z, c


@pytest.mark.parametrize("which", ["plain", "batch_norm"])
def test_float64_round_trip_closes_and_logdets_cancel(flow_sd, flow_sd_bn, which):
    sd = flow_sd if which == "plain" else flow_sd_bn
    z, c = _rows(sd)
    x, lp_s = fr.sample_and_log_prob(sd, z, c)
    lp_f, z_back = fr.log_prob(sd, x, c)
    print(f"{which}: round trip {np.abs(z_back - z).max():.1e}, log_prob gap {np.abs(lp_f - lp_s).max():.1e}, logdet {fr.logdet(sd):.3f}, "
          f"pose rms {np.sqrt((x ** 2).mean()):.2f}, |max| {np.abs(x).max():.1f}")
    assert np.abs(z_back - z).max() < 1e-10
    # sample_and_log_prob's log_prob is log_prob(samples): the inverse's log|det| is minus the forward's
    assert np.abs(lp_f - lp_s).max() < 1e-9
    assert np.abs(lp_s[0] - (-fr.LOG_2PI_HALF_D + fr.logdet(sd))) < 1e-12          # z = 0
    assert fr.has_batch_norm(fr.transform_keys(sd)[2]) == (which == "batch_norm")


def test_float32_run_stays_near_the_float64_run(flow_sd):
    z, c = _rows(flow_sd)
    x64, _ = fr.sample_and_log_prob(flow_sd, z, c)
    x32, lp32 = fr.sample_and_log_prob(flow_sd, z.astype(np.float32), c.astype(np.float32), np.float32)
    assert x32.dtype == np.float32
    z32 = fr.forward(flow_sd, x64.astype(np.float32), c.astype(np.float32), np.float32)
    e_s, e_f = np.abs(x32 - x64).max(), np.abs(z32 - fr.forward(flow_sd, x64.astype(np.float32), c.astype(np.float32))).max()
    print(f"float32 against float64: sampling {e_s:.1e}, forward {e_f:.1e}")
    assert e_s < 1e-3 and e_f < 1e-3


def test_synthetic_blocks_are_well_conditioned(flow_sd, flow_sd_bn):
    for sd in (flow_sd, flow_sd_bn):
        tk = fr.transform_keys(sd)
        for i, kind in enumerate(fr.infer_kinds(sd)):
            if kind == "lulinear":
                Lm, U = fr.lu_matrices(tk[i])
                cond = np.linalg.cond(Lm @ U, 2)
                print(f"transform {i}: cond2(L U) = {cond:.1f}")
                assert cond < 100


def test_entries_fill_the_triangles_row_major():
    p = {"lower_entries": np.arange(1, 10297, dtype=np.float64), "upper_entries": -np.arange(1, 10297, dtype=np.float64),
         "unconstrained_upper_diag": np.zeros(144)}
    Lm, U = fr.lu_matrices(p)
    assert Lm[1, 0] == 1 and Lm[2, 0] == 2 and Lm[2, 1] == 3 and Lm[143, 142] == 10296 and np.array_equal(np.diag(Lm), np.ones(144))
    assert U[0, 1] == -1 and U[0, 143] == -143 and U[1, 2] == -144 and U[142, 143] == -10296
    np.testing.assert_allclose(np.diag(U), np.log(2.0) + 1e-3)
    assert np.array_equal(np.triu(Lm, 1), np.zeros((144, 144))) and np.array_equal(np.tril(U, -1), np.zeros((144, 144)))


@pytest.mark.parametrize("tag", list(FLAGS))
@pytest.mark.parametrize("bn", [False, True])
def test_model_state_dict_is_the_two_manifests(tag, bn):
    from egohmr_amd.stage1 import ProHMRScene
    m = ProHMRScene(flow_batch_norm=bn, **FLAGS[tag])
    want = dict(syn.stage1_manifest(**FLAGS[tag]) + syn.stage1_flow_manifest(batch_norm=bn, **FLAGS[tag]))
    got = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    assert got == {k: tuple(s) for k, s in want.items()}


def test_kind_inference_agrees_and_follows_the_key_sets(flow_sd):
    from egohmr_amd import io as eio
    pre = "flow.flow._transform._transforms."
    assert fr.infer_kinds(flow_sd) == eio.flow_transform_kinds(flow_sd) == ["actnorm", "lulinear", "coupling"] * 4
    # the kinds come from the keys, not from the position: a chain stored in another order is reported in that order
    swapped = {}
    for k, v in flow_sd.items():
        i, name = k[len(pre):].split(".", 1)
        j = {0: 1, 1: 0}.get(int(i), int(i))
        swapped[f"{pre}{j}.{name}"] = v
    assert eio.flow_transform_kinds(swapped)[:3] == fr.infer_kinds(swapped)[:3] == ["lulinear", "actnorm", "coupling"]


def _t(sd):
    return {"state_dict": {k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}}


def test_loader_with_the_flow_loads_every_key_and_the_default_call_ignores_it(full_sd):
    from egohmr_amd import io as eio
    from egohmr_amd.stage1 import ProHMRScene, ProHMRSceneTransl
    extra = {"discriminator.fc1.weight": np.zeros((4, 4), np.float32), "smpl.betas": np.zeros((1, 10), np.float32), "initialized": np.array(True),
             "flow.flow._distribution._log_z": np.array(132.3, dtype=np.float64)}
    ck = _t({**full_sd, **extra})
    plain = eio.load_stage1_checkpoint(ProHMRSceneTransl(), ck)
    assert plain == sorted(k for k, _ in syn.stage1_manifest())                     # as before the flow existed: flow.flow.* ignored
    m = ProHMRScene()
    keys = eio.load_stage1_checkpoint(m, ck, flow=True)
    assert keys == sorted(full_sd)
    got = m.state_dict()
    for k in ("flow.flow._transform._transforms.0.log_scale", "flow.flow._transform._transforms.10.bias",
              "flow.flow._transform._transforms.11.transform_features", "flow.flow._transform._transforms.5.transform_net.blocks.1.context_layer.weight",
              "flow.fc_head.layers.0.weight"):
        assert np.array_equal(got[k].numpy(), full_sd[k]), k
    # the default call refuses a model that has the flow: its keys would be missing
    with pytest.raises(KeyError, match="flow.flow._transform._transforms.0.initialized"):
        eio.load_stage1_checkpoint(ProHMRScene(), ck)


def test_loader_refusals(full_sd, flow_sd):
    from egohmr_amd import io as eio
    from egohmr_amd.stage1 import ProHMRScene
    pre = "flow.flow._transform._transforms."
    m = ProHMRScene()
    before = {k: v.clone() for k, v in m.state_dict().items()}
    # affine coupling: a final layer of 144 rows
    bad = dict(full_sd)
    bad[pre + "2.transform_net.final_layer.weight"] = np.zeros((144, 1024), np.float32)
    with pytest.raises(ValueError, match=r"_transforms\.2 has a final_layer of 144 rows"):
        eio.load_stage1_checkpoint(m, _t(bad), flow=True)
    with pytest.raises(ValueError, match="144 rows"):
        fr.infer_kinds(bad)
    # an ActNorm that was never initialised
    bad = dict(full_sd)
    bad[pre + "3.initialized"] = np.array(False)
    with pytest.raises(ValueError, match=r"_transforms\.3 has initialized == False"):
        eio.load_stage1_checkpoint(m, _t(bad), flow=True)
    with pytest.raises(ValueError, match="initialized == False"):
        fr.infer_kinds(bad)
    # an unknown transform
    bad = {k: v for k, v in full_sd.items() if not k.startswith(pre + "4.")}
    bad[pre + "4.weight"] = np.zeros((144, 144), np.float32)
    with pytest.raises(KeyError, match=r"unknown flow transform .*_transforms\.4 with keys \['weight'\]"):
        eio.load_stage1_checkpoint(m, _t(bad), flow=True)
    with pytest.raises(KeyError, match="unknown transform"):
        fr.infer_kinds(bad)
    # another chain than the model's
    bad = {k: v for k, v in full_sd.items() if not k.startswith((pre + "9.", pre + "10.", pre + "11."))}
    with pytest.raises(KeyError, match="the flow's transforms are"):
        eio.load_stage1_checkpoint(m, _t(bad), flow=True)
    # a missing key, named
    gone = pre + "8.transform_net.blocks.1.linear_layers.0.bias"
    with pytest.raises(KeyError, match=gone.replace(".", r"\.")):
        eio.load_stage1_checkpoint(m, _t({k: v for k, v in full_sd.items() if k != gone}), flow=True)
    # BatchNorm keys the model was not built for, named
    bad = dict(full_sd)
    bad[pre + "2.transform_net.blocks.0.batch_norm_layers.0.weight"] = np.ones(1024, np.float32)
    with pytest.raises(KeyError, match="batch_norm_layers"):
        eio.load_stage1_checkpoint(m, _t(bad), flow=True)
    # a context width that does not match the flags: the head's, and (with a head that fits) the flow's own
    off = {**syn.make_stage1_state_dict(0, **ALL_OFF), **syn.make_stage1_flow_state_dict(0, **ALL_OFF)}
    with pytest.raises(ValueError, match="context flags"):
        eio.load_stage1_checkpoint(m, _t(off), flow=True)
    mixed = {**full_sd, **{k: v for k, v in off.items() if k.startswith("flow.flow.")}}
    with pytest.raises(ValueError, match=r"flow\.flow\..*context_layer\.weight is \(1024, 2560\), the model needs \(1024, 2566\)"):
        eio.load_stage1_checkpoint(m, _t(mixed), flow=True)
    # nothing was loaded in part
    after = m.state_dict()
    assert all(torch.equal(before[k], after[k]) for k in before)


def test_host_fold_matches_the_definition(flow_sd):
    """GlowFlow's host preparation (torch on the CPU: no kernel runs): the folded affine maps against ActNorm then LULinear in float64, A^-1 A = 1,
    and the constant log|det|."""
    from egohmr_amd.stage1 import GlowFlow
    f = GlowFlow(2566)
    f.load_state_dict({k[len("flow.flow."):]: torch.from_numpy(np.asarray(v)) for k, v in flow_sd.items()}, strict=True)
    w = f._weights(torch.device("cpu"))
    assert abs(w["logdet"] - fr.logdet(flow_sd)) < 1e-9
    tk = fr.transform_keys(flow_sd)
    x = np.random.Generator(np.random.PCG64(5)).normal(size=(4, 144))
    for l in range(4):
        a, lu = tk[3 * l], tk[3 * l + 1]
        Lm, U = fr.lu_matrices(lu)
        want = ((np.exp(a["log_scale"].astype(np.float64)) * x + a["shift"]) @ U.T) @ Lm.T + lu["bias"]
        At, Ainvt, c = (w["blocks"][l][k].numpy().astype(np.float64) for k in ("At", "Ainvt", "c"))
        assert At.shape == (144, 160) and not At[:, 144:].any() and not Ainvt[:, 144:].any()
        np.testing.assert_allclose(x @ At[:, :144] + c, want, rtol=0, atol=2e-5)
        np.testing.assert_allclose((want - c) @ Ainvt[:, :144], x, rtol=0, atol=2e-5)
        cp = tk[3 * l + 2]
        assert np.array_equal(w["blocks"][l]["idf"].numpy(), cp["identity_features"]) and np.array_equal(w["blocks"][l]["trf"].numpy(), cp["transform_features"])
    # the context product's slices: first layer and gates of every coupling, zero rows in the pad
    Wctx = w["Wctx"].numpy()
    assert Wctx.shape == (2592, 12 * 1024) and not Wctx[2566:].any()
    assert np.array_equal(Wctx[:2566, 7 * 1024:8 * 1024], tk[8]["transform_net.blocks.0.context_layer.weight"].T)
    assert np.array_equal(Wctx[:2566, 3 * 1024:4 * 1024], tk[5]["transform_net.initial_layer.weight"][:, 72:].T)


def test_index_lists_that_are_no_split_are_refused(flow_sd):
    from egohmr_amd.stage1 import GlowFlow
    f = GlowFlow(2566)
    sd = {k[len("flow.flow."):]: torch.from_numpy(np.asarray(v)) for k, v in flow_sd.items()}
    sd["_transform._transforms.5.transform_features"] = sd["_transform._transforms.5.identity_features"].clone()
    f.load_state_dict(sd, strict=True)
    with pytest.raises(ValueError, match="coupling 5"):
        f._weights(torch.device("cpu"))


def test_cpu_tensors_raise():
    from egohmr_amd._lib import EgoHMRHipError
    from egohmr_amd.stage1 import GlowFlow, ProHMRScene
    f = GlowFlow(2560)
    with pytest.raises(EgoHMRHipError):
        f.sample_and_log_prob(torch.zeros(2, 2560), num_samples=2)
    with pytest.raises(EgoHMRHipError):
        f.log_prob(torch.zeros(2, 1, 144), torch.zeros(2, 2560))
    with pytest.raises(EgoHMRHipError):
        ProHMRScene(smpl=object())({"img": torch.zeros(1, 3, 224, 224)})


def test_stage1_driver_with_body_models_needs_the_sampling_model():
    from egohmr_amd.driver import Stage1Driver
    from egohmr_amd.stage1 import ProHMRScene, ProHMRSceneTransl
    body = object()
    with pytest.raises(TypeError, match="need an egohmr_amd.stage1.ProHMRScene .*not ProHMRSceneTransl"):
        Stage1Driver(ProHMRSceneTransl(), body, body, body)
    with pytest.raises(ValueError, match="all three body models"):
        Stage1Driver(ProHMRScene(), body, None, body)
    assert Stage1Driver(ProHMRScene(), body, body, body).with_metrics and not Stage1Driver(ProHMRSceneTransl()).with_metrics


def test_kind_inference_reads_tensors_of_a_state_dict(flow_sd):
    """The model's own state dict holds tensors (on whatever device it lives): flags are read with bool(tensor.cpu()), shapes without a copy."""
    from egohmr_amd import io as eio
    from egohmr_amd.stage1 import ProHMRScene
    sd = ProHMRScene().state_dict()
    assert eio.flow_transform_kinds(sd) == ["actnorm", "lulinear", "coupling"] * 4
    sd["flow.flow._transform._transforms.9.initialized"] = torch.tensor(False)
    with pytest.raises(ValueError, match=r"_transforms\.9 has initialized == False"):
        eio.flow_transform_kinds(sd)


def _gemm_desc(**kw):
    from egohmr_amd import _lib
    base = dict(X=0x10000, gather=None, W=0x20000, bias=None, pro_scale=None, pro_shift=None, item=None, scatter=None, Y=0x30000, R=5, K=1024, N=1024, S=1,
                ldx=1024, ldw=1024, ldy=1024, ld_item=0, prologue=0, epilogue=0)
    base.update(kw)
    return C.byref(_lib.FlowGemmDesc(**base))


def test_flow_cabi_rejects_bad_arguments_without_a_gpu():
    """Every refusal runs before anything is launched (dummy addresses: nothing may be read or written through them)."""
    from egohmr_amd import _lib
    L = _lib.lib()
    assert L.ehm_flow_gemm(None, None) == -22 and b"bad argument" in L.ehm_last_error()
    for bad in (dict(X=None), dict(W=None), dict(Y=None), dict(R=0), dict(S=0), dict(N=0),
                dict(Y=0x10000),                                   # in place on X
                dict(K=68, ldx=68),                                # K % 8
                dict(N=72, ldw=72),                                # ldw % 32
                dict(N=72, ldw=64),                                # ldw < N
                dict(ldx=512),                                     # ldx < K without a gather list
                dict(ldx=1026),                                    # ldx % 4
                dict(X=0x10004),                                   # X not 16-byte aligned
                dict(prologue=4), dict(prologue=-1), dict(epilogue=5),
                dict(prologue=2, pro_scale=0x40000),               # BatchNorm without its shift
                dict(prologue=3),                                  # shift without its vector
                dict(epilogue=1), dict(epilogue=2),                # per-item term without `item`
                dict(epilogue=1, item=0x50000, ld_item=512),       # an item row shorter than N
                dict(epilogue=3), dict(epilogue=4),                # scatter without its list
                dict(ldy=512)):                                    # a Y row shorter than N
        assert L.ehm_flow_gemm(_gemm_desc(**bad), None) == -22, bad
        assert b"bad argument" in L.ehm_last_error() or b"ehm_flow_gemm" in L.ehm_last_error(), bad
    assert L.ehm_flow_finish(None, 0.0, 0x10000, None, None, None, None, 4, None) == -22
    assert L.ehm_flow_finish(0x10000, 0.0, None, None, None, None, None, 4, None) == -22
    assert L.ehm_flow_finish(0x10000, 0.0, 0x20000, None, None, None, None, 0, None) == -22
    assert L.ehm_flow_finish(0x10000, 0.0, 0x20000, 0x30000, None, None, None, 4, None) == -22      # the pose outputs: all four or none
    assert L.ehm_flow_context(None, None) == -22
    ctx = dict(img_feats=0x10000, scene_feats=0x20000, fx=0x30000, cam_cx=0x30000, cam_cy=0x30000, box_center=0x30000, box_size=0x30000, out=0x40000,
               fx_norm=1500.0, with_cam_center=1, with_bbox_info=1, with_focal_length=1, img_dim=2048, scene_dim=512, ctx_pad=2592, B=2)
    for bad in (dict(out=None), dict(B=0), dict(img_feats=None), dict(img_dim=0)):
        assert L.ehm_flow_context(C.byref(_lib.FlowContextDesc(**{**ctx, **bad})), None) == -22, bad
    assert L.ehm_flow_context(C.byref(_lib.FlowContextDesc(**{**ctx, "ctx_pad": 2560})), None) == -22
    assert b"shorter than the context (2566 columns)" in L.ehm_last_error()
