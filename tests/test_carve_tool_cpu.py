"""Host side of python -m rendernet_amd.tools.carve_voxels: the two argument forms, the pose of an image name, the silhouette
rule and the frame arithmetic, on synthetic arrays.  No GPU."""
import os

import numpy as np
import pytest

from rendernet_amd.tools import carve_voxels as CV


def test_the_two_argument_forms():
    a = CV.parse_args(["shots", "hull.binvox"])
    assert a.images_dir == "shots" and a.output == "hull.binvox" and a.from_voxels is None
    assert (a.size, a.background, a.threshold, a.tolerance, a.axes) == (64, "black", 8.0, 0, "x,y,z")
    a = CV.parse_args(["--from-voxels", "chair.binvox", "--views", "12", "out.obj", "--tolerance", "1"])
    assert a.images_dir is None and a.from_voxels == "chair.binvox" and a.views == 12 and a.output == "out.obj"
    assert a.threshold == 0.5 and a.tolerance == 1
    a = CV.parse_args(["shots", "hull.ply", "--size", "32", "--background", "white", "--threshold", "20"])
    assert (a.size, a.background, a.threshold) == (32, "white", 20.0)


@pytest.mark.parametrize("argv", [["shots"], ["a", "b", "c.binvox"], ["--from-voxels", "in.binvox", "shots", "out.binvox"],
                                  ["shots", "hull.stl"], ["shots", "hull.binvox", "--size", "48"],
                                  ["shots", "hull.binvox", "--tolerance", "-1"], ["shots", "hull.binvox", "--background", "grey"],
                                  ["--from-voxels", "in.binvox", "--views", "0", "out.binvox"],
                                  ["--from-voxels", "in.binvox", "--views", "256", "out.binvox"]])
def test_refused_arguments(argv, capsys):
    with pytest.raises(SystemExit):
        CV.parse_args(argv)
    assert "carve_voxels" in capsys.readouterr().err


def test_pose_of_name():
    p = CV.pose_of_name(os.path.join("some", "folder", "chair_p90.00_t30.00_r3.3.png"))
    assert p.dtype == np.float32 and np.allclose(p, [np.pi / 2, np.pi / 3, 1.0])
    p = CV.pose_of_name("model_p250.00_t60.00_r2.5_extra.png")
    assert np.allclose(p, [250 * np.pi / 180, np.pi / 6, 3.3 / 2.5])
    with pytest.raises(ValueError):
        CV.pose_of_name("chair.png")


def test_silhouette_rule():
    img = np.zeros((4, 4, 3), np.uint8)
    img[0, 0] = (0, 0, 9)                                        # one channel above the threshold
    img[0, 1] = (8, 8, 8)                                        # every channel AT the threshold: background
    img[1, 1] = (255, 255, 255)
    m = CV.silhouette(img, "black", 8)
    want = np.zeros((4, 4), bool)
    want[0, 0] = want[1, 1] = True
    assert m.dtype == bool and np.array_equal(m, want)
    assert np.array_equal(CV.silhouette(img, "white", 8), ~np.pad(np.ones((1, 1), bool), ((1, 2), (1, 2))))
    # grey and alpha: a single channel is its own colour, the alpha of an RGBA image is ignored
    assert np.array_equal(CV.silhouette(img[..., 2], "black", 8), want)
    rgba = np.concatenate([img, np.full((4, 4, 1), 255, np.uint8)], 2)
    assert np.array_equal(CV.silhouette(rgba, "black", 8), want)
    with pytest.raises(ValueError):
        CV.silhouette(img.astype(np.float32))
    v = CV.views_of_masks(want[None])
    assert v.dtype == np.int32 and v.shape == (1, 4, 4) and set(np.unique(v).tolist()) == {-1, 0} and v[0, 1, 1] == 0


def test_pixels_per_cell_of_an_image():
    assert CV.pixels_per_cell_of((512, 512, 3), 64) == 4 and CV.pixels_per_cell_of((256, 256), 64) == 2
    assert CV.pixels_per_cell_of((64, 64), 32) == 1 and CV.pixels_per_cell_of((2048, 2048), 128) == 8
    for shape, size in (((512, 256), 64), ((500, 500), 64), ((64, 64), 64), ((4096, 4096), 64)):
        with pytest.raises(ValueError):
            CV.pixels_per_cell_of(shape, size)


def test_list_and_read_images(tmp_path):
    from PIL import Image
    with pytest.raises(ValueError):
        CV.list_images(str(tmp_path))
    img = np.zeros((128, 128, 3), np.uint8)
    img[40:60, 30:90] = (200, 10, 10)
    for name in ("b_p10.00_t80.00_r3.3.png", "a_p200.00_t45.00_r3.0.png", "notes.txt"):
        if name.endswith(".png"):
            Image.fromarray(img).save(str(tmp_path / name))
        else:
            (tmp_path / name).write_text("not an image")
    assert CV.list_images(str(tmp_path)) == ["a_p200.00_t45.00_r3.0.png", "b_p10.00_t80.00_r3.3.png"]
    views, poses, f, names = CV.read_views(str(tmp_path), 32, "black", 8.0)
    assert f == 2 and views.shape == (2, 128, 128) and views.dtype == np.int32 and poses.shape == (2, 3)
    assert (views[:, 40:60, 30:90] == 0).all() and (views == 0).sum() == 2 * 20 * 60
    assert np.allclose(poses[0], [200 * np.pi / 180, np.pi / 4, 1.1])
    with pytest.raises(ValueError):
        CV.read_views(str(tmp_path), 128, "black", 8.0)            # 128 pixels cannot frame a 128^3 grid
    Image.fromarray(np.zeros((64, 64, 3), np.uint8)).save(str(tmp_path / "c_p0.00_t90.00_r3.3.png"))
    with pytest.raises(ValueError):
        CV.read_views(str(tmp_path), 32, "black", 8.0)             # sides differ
