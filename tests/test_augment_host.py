"""The host side of the training / validation path, without a GPU: the random draws of `sample_params` against the reference's own
statements (utils/data.py:69-80, 26-33), the CPU restatement of adjust_sharpness that the GPU tests compare with, the table the
binding hands to the library, and the `validate` sub-command's argument handling and refusals."""
import os

import numpy as np
import pytest
import torch

from tests import augment_common as ac

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, "color-transfer_amd", "configs")


# ---- 1. the draws -----------------------------------------------------------------------------------------------------------------------
def _reference_draws(height, width, crop, max_magnitude=0.5):
    """utils/data.py:69-80 and 26-33, statement by statement, without the image work between them"""
    top = np.random.randint(0, height - crop[-2])
    left = np.random.randint(0, width - crop[-1])
    swap = np.random.random() > 0.5
    vflip = np.random.random() > 0.5
    fn_idx = torch.randperm(6)
    brightness_factor = np.random.uniform(1 - max_magnitude, 1 + max_magnitude)
    contrast_factor = np.random.uniform(1 - max_magnitude, 1 + max_magnitude)
    saturation_factor = np.random.uniform(1 - max_magnitude, 1 + max_magnitude)
    hue_factor = np.random.uniform(-max_magnitude, max_magnitude)
    gamma = np.random.uniform(1 - max_magnitude, 1 + max_magnitude)
    sharpness_factor = np.random.uniform(1 - max_magnitude, 1 + max_magnitude)
    by_id = [("brightness", brightness_factor), ("contrast", contrast_factor), ("saturation", saturation_factor), ("hue", hue_factor),
             ("gamma", gamma), ("sharpness", sharpness_factor)]
    return {"top": top, "left": left, "swap_hflip": bool(swap), "vflip": bool(vflip), "ops": [by_id[int(i)] for i in fn_idx]}


@pytest.mark.parametrize("seed", [0, 20240607])
@pytest.mark.parametrize("extra", [1, 2], ids=["one_pixel_larger", "two_pixels_larger"])
def test_sample_params_draws_what_the_reference_draws(seed, extra):
    from utils.data import SyntheticTrainVal
    crop = (19, 23)
    ds = SyntheticTrainVal(n_images=3, height=crop[0] + extra, width=crop[1] + extra, crop_size=crop, image_repeats=4)
    assert len(ds) == 12
    indices = [0, 5, 11, 3, 3, 7, 1, 10, 2, 6, 9, 4]
    np.random.seed(seed)
    torch.manual_seed(seed)
    want = [_reference_draws(crop[0] + extra, crop[1] + extra, crop) for _ in indices]
    np.random.seed(seed)
    torch.manual_seed(seed)
    got = [ds.sample_params(i) for i in indices]
    assert got == want                                       # float64 strengths included, bit for bit
    for key in ("top", "left"):                              # 0 and the largest legal corner, extra - 1 (numpy's high is exclusive)
        assert {p[key] for p in got} == set(range(extra))
    assert {p["swap_hflip"] for p in got} == {False, True} and {p["vflip"] for p in got} == {False, True}
    assert len({tuple(k for k, _ in p["ops"]) for p in got}) > 6                       # orders differ between samples
    for p in got:
        assert sorted(k for k, _ in p["ops"]) == sorted(ac.KINDS[1:])
        for kind, value in p["ops"]:
            assert (-0.5 <= value <= 0.5) if kind == "hue" else (0.5 <= value <= 1.5)


def test_a_source_no_larger_than_the_crop_raises_numpys_error():
    from utils.data import SyntheticTrainVal
    for h, w in ((19, 40), (40, 23), (18, 40)):
        with pytest.raises(ValueError):
            SyntheticTrainVal(1, h, w, crop_size=(19, 23), image_repeats=1).sample_params(0)


def test_file_dataset_lists_and_length(tmp_path):
    from PIL import Image
    from utils.data import ArtificialTrainValDataset, DataModule
    (tmp_path / "Validation").mkdir()
    rng = np.random.default_rng(0)
    for name in ("b_L", "a_R", "a_L", "b_R"):
        Image.fromarray(rng.integers(0, 256, (30, 44, 3), dtype=np.uint8)).save(tmp_path / "Validation" / (name + ".png"))
    ds = ArtificialTrainValDataset(tmp_path / "Validation", crop_size=[16, 24], image_repeats=3)
    assert len(ds) == 6 and [p.name for p in ds.gts] == ["a_L.png", "b_L.png"] and [p.name for p in ds.references] == ["a_R.png", "b_R.png"]
    assert ds.source_size(1) == (30, 44)
    host, p = ds.host_frames(4)                              # sample 4 = image 4 // 3
    assert host["gt"].shape == (3, 30, 44) and host["gt"].dtype == torch.uint8 and 0 <= p["top"] < 14 and 0 <= p["left"] < 20
    dm = DataModule(data_dir=str(tmp_path), crop_size=[16, 24], image_repeats=3, batch_size=4)
    art, real = dm.val_dataloader()
    assert len(art) == 6 and art.batch_size == 4 and real.batch_size == 1
    with pytest.raises(ValueError):
        DataModule(data_dir=str(tmp_path)).val_dataloader()                            # no crop_size
    with pytest.raises(ValueError):
        DataModule(crop_size=[16, 24]).val_dataloader()                                # no directory and no `synthetic: trainval`


# ---- 2. the sharpness restatement -------------------------------------------------------------------------------------------------------
def test_sharpness_restatement_properties():
    g = torch.Generator().manual_seed(5)
    img = torch.randint(0, 256, (3, 9, 13), generator=g, dtype=torch.uint8)
    const = torch.full((3, 9, 13), 97, dtype=torch.uint8)
    for factor in (0.0, 0.3, 0.5, 1.0, 1.5, 2.0):
        assert torch.equal(ac.adjust_sharpness(const, factor), const)
    assert torch.equal(ac.adjust_sharpness(img, 1.0), img)
    blurred = ac.adjust_sharpness(img, 0.0)
    assert torch.equal(blurred, ac.blurred_degenerate_image(img))
    border = torch.ones(9, 13, dtype=torch.bool)
    border[1:-1, 1:-1] = False
    assert torch.equal(blurred[:, border], img[:, border]) and not torch.equal(blurred, img)
    for shape in ((3, 2, 7), (3, 7, 2)):
        small = torch.randint(0, 256, shape, generator=g, dtype=torch.uint8)
        assert torch.equal(ac.adjust_sharpness(small, 1.7), small)
    with pytest.raises(ValueError):
        ac.adjust_sharpness(img, -0.1)


def test_sharpness_restatement_on_a_hand_computed_example():
    plane = torch.tensor([[10, 20, 30], [40, 200, 60], [70, 80, 90]], dtype=torch.uint8)
    img = torch.stack([plane, plane.flip(0), torch.full((3, 3), 7, dtype=torch.uint8)])
    # the ring adds up to 400, the centre counts five times: (400 + 5 * 200) / 13 = 107.69 -> 108; the flipped plane has the same sum
    want0 = plane.clone()
    want0[1, 1] = 108
    assert torch.equal(ac.adjust_sharpness(img, 0.0), torch.stack([want0, want0.flip(0), img[2]]))
    # factor 2: 2 * 200 - 108 = 292 -> clamped to 255; factor 0.5: 100 + 54 = 154; the border and the constant plane stay
    for factor, centre in ((2.0, 255), (0.5, 154), (1.5, 246)):
        want = plane.clone()
        want[1, 1] = centre
        assert torch.equal(ac.adjust_sharpness(img, factor), torch.stack([want, want.flip(0), img[2]])), factor


def test_augment_table_layout():
    import ct_hip
    t = ct_hip.augment_table([ac.params(3, 4, True, False, [("hue", 0.25), ("sharpness", 1.3), (2, 0.7)]), ac.params()])
    assert t.dtype.itemsize == 144 and t.shape == (2,)
    raw = np.frombuffer(t.tobytes(), dtype=np.int32)
    assert raw[:12].tolist() == [3, 4, 1, 0, 3, 4, 6, 2, 0, 0, 0, 0]
    doubles = np.frombuffer(t.tobytes(), dtype=np.float64)
    assert doubles[6:9].tolist() == [0.25, 1.3, 0.7] and doubles[12:15].tolist() == [1.0 - 0.25, 1.0 - 1.3, 1.0 - 0.7]
    assert int(t[1]["n_ops"]) == 0
    with pytest.raises(ValueError):
        ct_hip.augment_table([ac.params(ops=[("gamma", 1.0)] * 7)])
    assert ct_hip.AUGMENT_KINDS["sharpness"] == 6 and [ct_hip.AUGMENT_KINDS[k] for k in ac.KINDS] == list(range(7))


# ---- 3. `validate`: arguments and refusals ----------------------------------------------------------------------------------------------
def test_validate_refusals(monkeypatch):
    from utils import cli
    monkeypatch.delenv("CT_CLI_DEVICE", raising=False)
    data = ["--data.synthetic", "trainval", "--data.crop_size", "[64, 96]"]
    with pytest.raises(SystemExit) as e:                     # the Runner has no validation_step, as in the reference
        cli.main(["validate", "--config", os.path.join(CFG, "others.yaml")] + data)
    assert "validation_step" in str(e.value) and "Runner" in str(e.value)
    with pytest.raises(SystemExit) as e:                     # DCMCS3DI lacks the three PAM losses
        cli.main(["validate", "--config", os.path.join(CFG, "dcmcs3di.yaml")] + data)
    assert all(name in str(e.value) for name in ("Photometric Loss", "Cycle Loss", "Smoothness Loss"))
    with pytest.raises(SystemExit) as e:
        cli.main(["validate", "--config", os.path.join(CFG, "dmsct.yaml"), "--inference.scale_factor", "0.75"] + data)
    assert "inference" in str(e.value)
    with pytest.raises(SystemExit) as e:
        cli.main(["validate", "--config", os.path.join(CFG, "dmsct.yaml"), "--data.batch_size"])
    assert "dangling" in str(e.value)
    monkeypatch.setenv("CT_CLI_DEVICE", "cpu")
    with pytest.raises(SystemExit) as e:
        cli.main(["validate", "--config", os.path.join(CFG, "dmsct.yaml")] + data)
    assert "CT_CLI_DEVICE=cpu" in str(e.value)


def test_dcmcs3di_validation_step_names_what_it_lacks():
    from methods.dcmcs3di import DCMCS3DI
    with pytest.raises(NotImplementedError) as e:
        DCMCS3DI.validation_step(None, {})
    assert all(name in str(e.value) for name in ("Photometric", "Cycle", "Smoothness"))


def test_validate_reads_its_data_arguments():
    from utils import cli
    from utils.data import DataModule
    cfg, ckpt, opts = cli._parse(["validate", "--config", os.path.join(CFG, "dmsct.yaml"), "--ckpt_path", "w.ckpt", "--data.synthetic", "trainval",
                                  "--data.crop_size", "[64, 96]", "--data.image_repeats", "2", "--data.batch_size", "2", "--data.n_frames", "2",
                                  "--data.height", "96", "--data.width", "160", "--seed_everything", "5"])
    assert ckpt == "w.ckpt" and not opts and cfg["seed_everything"] == 5 and cfg["model"]["class_path"] == "methods.dmsct.DMSCT"
    art, real = DataModule(**cfg["data"]["init_args"]).val_dataloader()
    assert len(art) == 4 and art.batch_size == 2 and art.dataset.crop_size == (64, 96) and art.dataset.source_size(0) == (96, 160)
    assert len(real) == 2 and real.batch_size == 1
