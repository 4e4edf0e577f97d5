"""GPU: egohmr_amd.jpeg.JpegDecoder.decode (host Huffman stage + csrc/jpeg.hip) against the committed pixels of tests/golden/jpeg_pixels.npz -
PIL's decode of the same files, i.e. libjpeg's ISLOW IDCT, fancy upsampling and colour tables - and BatchBuilder.build on encoded frames
against the same call on the decoded ones.  The rule is integer, so every bar is equality (maximum difference 0, identical bits).  Every test
here fails without the feature: the module and the entry points do not exist on the parent."""
import os
import random
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_jpeg_golden import BATCH, FIXTURES  # noqa: E402
from egohmr_amd import synthetic as syn  # noqa: E402

pytestmark = pytest.mark.gpu
NAMES = list(FIXTURES)


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def pixels(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "jpeg_pixels.npz")))


@pytest.fixture(scope="module")
def decoder(dev):
    from egohmr_amd import JpegDecoder
    return JpegDecoder(dev, threads=4)


def load(golden_dir, name):
    with open(os.path.join(golden_dir, "jpeg", name + ".jpg"), "rb") as f:
        return f.read()


@pytest.mark.parametrize("name", NAMES)
def test_decode_equals_the_committed_pixels(decoder, golden_dir, pixels, name):
    out = decoder.decode([load(golden_dir, name)])
    assert out.is_cuda and out.dtype == torch.uint8 and tuple(out.shape) == (1,) + pixels[name].shape
    got = out[0].cpu().numpy()
    diff = int(np.abs(got.astype(np.int32) - pixels[name].astype(np.int32)).max())
    print(f"{name}: maximum difference {diff}")
    assert diff == 0


def test_batch_of_three_qualities_and_repeatability(decoder, golden_dir, pixels):
    paths = [os.path.join(golden_dir, "jpeg", n + ".jpg") for n in BATCH]                # paths this time, bytes above
    a = decoder.decode(paths)
    b = decoder.decode([load(golden_dir, n) for n in BATCH])
    torch.cuda.synchronize()
    assert tuple(a.shape) == (3, 48, 64, 3)
    for i, n in enumerate(BATCH):
        assert np.array_equal(a[i].cpu().numpy(), pixels[n]), n
    assert torch.equal(a, b)
    # the same frame at three places of a batch, after a call of another geometry used the workspace
    decoder.decode([load(golden_dir, "p24x520_420")])
    c = decoder.decode([paths[2], paths[0], paths[2]])
    assert torch.equal(c[0], a[2]) and torch.equal(c[1], a[0]) and torch.equal(c[2], a[2])


def test_mixed_geometries_and_refused_files_raise(decoder, golden_dir):
    from egohmr_amd import EgoHMRHipError
    with pytest.raises(ValueError, match=r"item 0 is 48x64.*item 1 is 56x72"):
        decoder.decode([load(golden_dir, BATCH[0]), load(golden_dir, "p56x72_420")])
    with pytest.raises(ValueError, match="sampling 2x2.*sampling 1x1"):                   # same size, another sampling
        decoder.decode([load(golden_dir, "p56x72_420"), _with_444_header(golden_dir)])
    with pytest.raises(EgoHMRHipError, match=r"item 1 .*progressive"):
        decoder.decode([load(golden_dir, BATCH[0]), load(golden_dir, "progressive32x32")])


def _with_444_header(golden_dir):
    """The 56x72 4:2:0 fixture with the luma sampling byte of its frame header set to 1x1: a valid header of the same size and another
    sampling (its scan is never reached: the geometry check comes first)."""
    data = bytearray(load(golden_dir, "p56x72_420"))
    sof = data.index(b"\xff\xc0")
    assert data[sof + 11] == 0x22
    data[sof + 11] = 0x11
    return bytes(data)


def _items(B, rng):
    kp2 = np.concatenate([rng.uniform(5, 60, (B, 25, 2)), rng.uniform(0.2, 1.0, (B, 25, 1))], -1)
    return dict(frame_index=np.arange(B), center=np.float32([[36.4, 27.8], [33.1, 30.2]])[:B], bbox_size=np.float32([44.0, 38.0])[:B],
                keypoints_2d=kp2, keypoints_3d=rng.normal(0, 0.4, (B, 24, 3)),
                smpl_params=dict(global_orient=rng.normal(0, 0.3, (B, 3)).astype(np.float32), body_pose=rng.normal(0, 0.2, (B, 69)).astype(np.float32),
                                 betas=rng.normal(0, 0.5, (B, 10)).astype(np.float32), transl=np.float32([[0.1, -0.2, 2.5], [-0.3, 0.1, 3.1]])[:B]),
                gender=np.array([0, 1])[:B], fx=np.full(B, 90.0), fy=np.full(B, 90.0), cx=np.full(B, 36.0), cy=np.full(B, 28.0),
                scene=rng.normal(0, 1, (B, 64, 3)).astype(np.float32))


def _same(a, b, path=""):
    if isinstance(a, dict):
        assert list(a) == list(b), path
        for k in a:
            _same(a[k], b[k], f"{path}/{k}")
    else:
        assert a.dtype == b.dtype and a.device == b.device and torch.equal(a, b), path


@pytest.mark.parametrize("augment", [None, "draw"])
def test_builder_on_encoded_frames_equals_decoded_frames(dev, golden_dir, pixels, augment):
    from egohmr_amd import BatchBuilder
    from egohmr_amd.smpl import SMPL
    names = ["p56x72_420", "p56x72_420_opt"]
    models = (SMPL(syn.make_smpl_asset(1), gender="male").to(dev), SMPL(syn.make_smpl_asset(2), gender="female").to(dev)) if augment else (None, None)
    bld = BatchBuilder(dev, img_size=32, smpl_male=models[0], smpl_female=models[1])
    kw = _items(2, np.random.default_rng(2401))
    outs = []
    for frames in ([load(golden_dir, n) for n in names], np.stack([pixels[n] for n in names]),
                   [os.path.join(golden_dir, "jpeg", n + ".jpg") for n in names]):
        np.random.seed(5)
        random.seed(5)
        outs.append(bld.build(frames, augment=augment, **kw))
    torch.cuda.synchronize()
    assert tuple(outs[0]["img"].shape) == (2, 3, 32, 32) and bool(torch.isfinite(outs[0]["img"]).all())
    _same(outs[0], outs[1])
    _same(outs[2], outs[1])
