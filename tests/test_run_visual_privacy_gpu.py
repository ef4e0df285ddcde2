"""run_privacy's visual stage with `detector: boxes` end to end on the GPU: frames from PNG files
in nested directories, boxes from a file, against tests/blur_mirror.py computed from the same
files; and the synthetic mode."""
import sys

import numpy as np
import pytest
import yaml

import blur_mirror as BM

pytestmark = pytest.mark.gpu


def _tree(root):
    from PIL import Image
    rng = np.random.default_rng(21)
    frames = {}
    for rel, hw in (("a/f0.png", (24, 40)), ("a/f1.png", (24, 40)), ("a/deep/f2.png", (30, 70)), ("b/f3.png", (30, 70)),
                    ("b/f4.png", (24, 40)), ("f5.png", (30, 70))):
        arr = rng.integers(0, 256, hw + (3,), dtype=np.uint8)
        p = root / rel
        p.parent.mkdir(parents=True, exist_ok=True)
        Image.fromarray(arr).save(p)
        frames[rel] = arr
    boxes = {"a/f0.png": [(4, 4, 10, 12)], "a/deep/f2.png": [(-5, 10, 30, 15), (60, 0, 20, 40)],
             "b/f4.png": [(0, 0, 40, 24)], "f5.png": [(10, 10, 0, 5)]}
    lines = ["# test boxes", "path,x,y,w,h"]
    for rel, bs in boxes.items():
        lines += [f"{rel},{x},{y},{w},{h}" for x, y, w, h in bs]
    lines.append("gone/missing.png,1,1,5,5")
    bf = root.parent / "boxes.csv"
    bf.write_text("\n".join(lines) + "\n")
    return frames, boxes, bf


def test_main_with_boxes_matches_the_mirror(tmp_path):
    from PIL import Image
    from ssl_mae_amd import run_privacy as RP
    from ssl_mae_amd import visual_privacy as V
    root = tmp_path / "frames"
    frames, boxes, bf = _tree(root)
    cfg = {"visual_privacy": {"enabled": True, "detector": "boxes", "frame_root": str(root), "boxes_file": str(bf),
                              "blur_kernel": 14, "overwrite": True, "batch_frames": 4, "save_examples": 3},
           "feature_privacy": {"enabled": False}, "runtime": {"seed": 3}}
    cfg_file = tmp_path / "privacy.yaml"
    cfg_file.write_text(yaml.safe_dump(cfg))

    # the mirror, from the same files in scan order
    rels = sorted(frames, key=lambda r: (root / r))
    w = V.gaussian_weights(15)
    stats, after = [], {}
    for rel in rels:
        fr = frames[rel]
        h, wd = fr.shape[:2]
        b = np.asarray(boxes.get(rel, []), np.int64).reshape(-1, 4)
        out = BM.box_blur_batch(fr.reshape(-1), [[0, h, wd]], b, [0, len(b)], w, h, wd, np.zeros(fr.size, np.uint8))
        after[rel] = out.reshape(h, wd, 3)
        stats.append(BM.region_stats(fr.reshape(-1), out, [[0, h, wd]], b, [0, len(b)], h, wd)[0].tolist())
    want = V.summarise(stats, [frames[r].shape[:2] for r in rels], [len(boxes.get(r, [])) for r in rels])
    assert want["frames_with_box"] == 3 and want["total_frames"] == 6 and want["avg_boxes"] == 5 / 6

    texts = []
    for run in ("a", "b"):
        save = tmp_path / run
        res = RP.main(["--config", str(cfg_file), "--save_dir", str(save)])
        assert res["rows"] == [] and res["visual"]["csv"] == save / "visual_privacy.csv"
        lines = (save / "visual_privacy.csv").read_text().splitlines()
        assert lines[0] + "\n" == V.CSV_HEADER and len(lines) == 2
        row = dict(zip(V.CSV_COLUMNS, lines[1].split(",")))
        out_root = tmp_path / "frames_frames_privacy"
        assert row["frame_root"] == str(root) and row["overwrite_saved_root"] == str(out_root)
        assert row["total_frames"] == "6" and row["frames_with_box"] == "3" and row["blur_kernel"] == "15"
        for c in ("avg_boxes", "box_pixel_fraction", "psnr_box_db", "detail_retained"):
            assert float(row[c]) == round(want[c], 6), c
            assert res["visual"][c] == want[c], c
        assert float(row["seconds"]) > 0
        for rel in rels:                             # the saved frames are the mirror's, bit for bit
            with Image.open(out_root / rel) as im:
                assert np.array_equal(np.asarray(im.convert("RGB")), after[rel]), rel
        with Image.open(save / "visual_privacy_examples.jpg") as im:
            assert im.size == (3 * 70, 2 * 30)       # three examples at the first one's size, before above after
        log = (save / "privacy.log").read_text()
        assert "1 listed paths match no sampled frame" in log and "Saved visual privacy CSV" in log
        texts.append([v for c, v in row.items() if c != "seconds"])
    assert texts[0] == texts[1]                      # a second run differs only in `seconds`
    assert "cv2" not in sys.modules


def test_synthetic_mode(tmp_path):
    from ssl_mae_amd import run_privacy as RP
    from ssl_mae_amd import visual_privacy as V
    cfg_file = tmp_path / "privacy.yaml"
    cfg_file.write_text(yaml.safe_dump({"visual_privacy": {"enabled": True, "detector": "boxes", "max_images": 6,
                                                           "blur_kernel": 31, "batch_frames": 4, "save_examples": 0},
                                        "feature_privacy": {"enabled": False}}))
    res = RP.main(["--config", str(cfg_file), "--save_dir", str(tmp_path / "out")])
    lines = (tmp_path / "out" / "visual_privacy.csv").read_text().splitlines()
    row = dict(zip(V.CSV_COLUMNS, lines[1].split(",")))
    assert lines[0] + "\n" == V.CSV_HEADER and row["frame_root"] == "synthetic" and row["total_frames"] == "6"
    assert row["frames_with_box"] == "6" and float(row["avg_boxes"]) == 1.5 and row["overwrite_saved_root"] == ""
    assert 0.0 < float(row["detail_retained"]) < 0.05 and 5.0 < float(row["psnr_box_db"]) < 20.0    # noise, blurred
    assert 0.0 < float(row["box_pixel_fraction"]) <= (96 * 96 + 48 * 48) / (240 * 320)
    assert not (tmp_path / "out" / "visual_privacy_examples.jpg").exists()
    assert res["visual"]["total_frames"] == 6 and "cv2" not in sys.modules
