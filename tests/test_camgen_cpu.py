"""CPU checks of the stand-alone CAM generation: the numpy restatement of Pillow's 8-bit bicubic resize that
the kernel is written against, the host-side helpers of clip/generate_cams.py and the new ABI symbols."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import preprocess_ref as PR  # noqa: E402

import weclip_vit_comer_amd  # noqa: E402,F401
from weclip_vit_comer_amd import _lib  # noqa: E402


@pytest.fixture(scope="module")
def fx(golden):
    return golden("clip_preprocess.npz")


def _cases(fx):
    return range(int(fx["n_cases"]))


def test_fixture_covers_the_cases_of_the_issue(fx):
    kinds = set()
    for i in _cases(fx):
        H0, W0 = fx[f"c{i}_src"].shape[:2]
        h, w = fx[f"c{i}_u8"].shape[:2]
        s = float(fx[f"c{i}_scale"])
        assert (h, w) == PR.target_size(H0, W0, s) and h % 16 == 0 and w % 16 == 0
        if s != 1.0:
            kinds.add(("scale", s))
        elif (h, w) == (H0, W0):
            kinds.add("none")
        elif h != H0 and w != W0:
            kinds.add("both")
        else:
            kinds.add("one")
        if W0 == 1:
            kinds.add("1wide")
        if H0 == 3:
            kinds.add("3high")
    assert kinds >= {"none", "one", "both", ("scale", 0.5), ("scale", 2.0), "1wide", "3high"}


def test_numpy_bicubic_equals_pillow_fixture_bit_for_bit(fx):
    for i in _cases(fx):
        src, want = fx[f"c{i}_src"], fx[f"c{i}_u8"]
        got = PR.bicubic_resize_u8(src, *want.shape[:2])
        assert np.array_equal(got, want), f"case {i}: {np.count_nonzero(got != want)} differing bytes"


def test_numpy_normalise_and_flip_equal_the_reference_tensors(fx):
    for i in _cases(fx):
        out = PR.clip_normalize(fx[f"c{i}_u8"])
        assert np.array_equal(out.view(np.uint32), fx[f"c{i}_out"].view(np.uint32)), f"case {i}"
        assert np.array_equal(out[:, :, ::-1].view(np.uint32), fx[f"c{i}_flip"].view(np.uint32)), f"case {i}"


def test_numpy_bicubic_equals_live_pillow_on_random_sizes():
    Image = pytest.importorskip("PIL.Image")
    rng = np.random.default_rng(5)
    for _ in range(20):
        H0, W0, h, w = (int(v) for v in rng.integers(1, 65, 4))
        if max(H0 / h, W0 / w) > 8:          # the documented limit of the kernel (down-scaling by at most 8)
            h, w = max(h, -(-H0 // 8)), max(w, -(-W0 // 8))
        src = rng.integers(0, 256, (H0, W0, 3), dtype=np.uint8)
        want = np.asarray(Image.fromarray(src).resize((w, h), Image.BICUBIC))
        assert np.array_equal(PR.bicubic_resize_u8(src, h, w), want), (H0, W0, h, w)


def test_scale_cam_restatement_basics():
    cam = np.random.default_rng(0).random((4, 6)).astype(np.float32)
    out = PR.scale_cam_resize_f16(cam, 4, 6)                          # same size: the bilinear resize is the identity
    ref = ((cam - cam.min()) / (np.float32(1e-7) + (cam - cam.min()).max())).astype(np.float16)
    assert out.dtype == np.float16 and np.array_equal(out, ref)
    up = PR.scale_cam_resize_f16(cam, 37, 50)
    assert up.shape == (37, 50) and up.min() >= 0 and up.max() <= 1
    assert PR.f16_ulp_distance(np.float16([1.0, -0.0]), np.float16([1.001, 0.0])).tolist() == [1, 0]


def test_bilinear_and_scale_cam_restatements_equal_the_reference_fixture(golden):
    """The numpy output stage that GPU tests use as a reference is itself pinned to the recorded scale_cam_image / cv2.resize:
    1 fp16 ulp, and 8 fp32 eps of the map's maximum for the plain resize (bound derived in tests/test_camgen_gpu.py)."""
    g = golden("cam_scale_resize.npz")
    for i in range(int(g["n_pairs"])):
        cam, want, plain = g[f"p{i}_cam"], g[f"p{i}_out"], g[f"p{i}_plain"]
        got = PR.scale_cam_resize_f16(cam, *want.shape)
        assert got.dtype == np.float16 and PR.f16_ulp_distance(got, want).max() <= 1, f"pair {i}"
        e = np.abs(PR.bilinear_resize_f32(cam, *plain.shape) - plain).max()
        assert e <= 8 * np.finfo(np.float32).eps * np.abs(plain).max(), (i, e)


def test_perform_fixture_satisfies_the_input_conditions(golden):
    """camgen_tiny.npz: >= 4 images, two of one size, two sizes that are no multiples of 16 in different ways, 1 / 2 / 3 labels,
    no quantised CAM value within 1 of the box threshold, refined maxima >= 1e-3 (tests/golden/make_camgen_golden.py)."""
    g = golden("camgen_tiny.npz")
    n = int(g["n_images"])
    sizes = [g[f"img{i}_src"].shape[:2] for i in range(n)]
    assert n >= 4 and len(set(sizes)) < n
    assert len({(h % 16 != 0, w % 16 != 0, h, w) for h, w in sizes if h % 16 or w % 16}) >= 2
    assert {len(g[f"img{i}_labels"]) for i in range(n)} >= {1, 2, 3}
    for tag, thr in (("voc", 0.4), ("coco", 0.7)):
        for i in range(n):
            assert g[f"{tag}{i}_keys"].tolist() == g[f"img{i}_labels"].tolist()
            assert g[f"{tag}{i}_attn_highres"].dtype == np.float16
            assert g[f"{tag}{i}_attn_highres"].shape == (len(g[f"img{i}_labels"]),) + sizes[i]
            for k, cam in enumerate(g[f"{tag}{i}_gray"]):
                q = (cam * 255).astype(np.uint8).astype(np.int64)
                assert not (np.abs(q - int(thr * q.max())) <= 1).any()
                assert g[f"{tag}{i}_refined"][k].max() >= 1e-3
                hi = PR.scale_cam_resize_f16(g[f"{tag}{i}_refined"][k], *sizes[i])
                assert PR.f16_ulp_distance(hi, g[f"{tag}{i}_attn_highres"][k]).max() <= 1
            assert np.array_equal(PR.clip_normalize(PR.bicubic_resize_u8(g[f"img{i}_src"], *g[f"img{i}_input"].shape[1:])),
                                  g[f"img{i}_input"])


def test_worker_command_lines_and_spawn(tmp_path):
    """`--num_workers 2` started the documented way (`python -m <package>.clip.generate_cams_*`): the children are started by the
    driver's importable module name with their worker ids, and the parent exits 0 (an empty split: no worker touches the GPU)."""
    from weclip_vit_comer_amd.clip import generate_cams as G
    from weclip_vit_comer_amd.clip import generate_cams_coco14 as C
    from weclip_vit_comer_amd.clip import generate_cams_voc12 as V
    assert V.MODULE == "weclip_vit_comer_amd.clip.generate_cams_voc12" and C.MODULE == "weclip_vit_comer_amd.clip.generate_cams_coco14"
    cmds = G.worker_commands(3, V.MODULE, ["--img_root", "x"])
    assert [c[1:3] for c in cmds] == [["-m", V.MODULE]] * 3 and all(c[0] == sys.executable for c in cmds)
    assert [c[3:] for c in cmds] == [["--img_root", "x", "--num_workers", "3", "--worker_id", str(i)] for i in range(3)]
    assert len(G.worker_commands(40, V.MODULE, [])) == G.MAX_WORKERS == 16
    capped = G.worker_commands(40, V.MODULE, ["--num_workers", "40", "--model", "m", "--num_workers=40"])[5]
    assert capped[3:] == ["--model", "m", "--num_workers", "16", "--worker_id", "5"]
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    split = tmp_path / "split.txt"
    split.write_text("")
    for mod in (V.MODULE, C.MODULE):
        r = subprocess.run([sys.executable, "-W", "ignore", "-m", mod, "--img_root", str(tmp_path), "--split_file", str(split),
                            "--cam_out_dir", str(tmp_path / "out"), "--model", "none", "--num_workers", "2"],
                           capture_output=True, text=True, cwd=root)
        assert r.returncode == 0, r.stderr
    # a child that fails makes the parent fail
    bad = subprocess.run([sys.executable, "-c", "import sys; from weclip_vit_comer_amd.clip import generate_cams as G; "
                          "G.spawn_workers(2, 'weclip_vit_comer_amd.clip.no_such_driver', [])"], capture_output=True, text=True, cwd=root)
    assert bad.returncode != 0 and "CAM workers failed" in bad.stderr


def test_size_rounding_buckets_and_split():
    from weclip_vit_comer_amd.clip import generate_cams as G
    assert G.target_size(375, 500) == (384, 512) and G.target_size(384, 512) == (384, 512)
    assert G.target_size(333, 500, 0.5) == (176, 256) and G.target_size(45, 37, 2.0) == (96, 80)
    for H0 in range(1, 70):
        assert G.target_size(H0, 1) == PR.target_size(H0, 1)
    sizes = [(375, 500), (500, 375), (375, 500), (333, 500), (375, 500)]
    labels = [[1], [2, 3], [4], [], [5]]
    buckets, skipped = G.bucket_images(sizes, labels, max_bucket=2)
    assert buckets == [[0, 2], [4], [1]] and skipped == [3]
    assert G.bucket_images(sizes, labels, max_bucket=16)[0] == [[0, 2, 4], [1]]
    data = list(range(11))
    for n in (1, 2, 3, 4, 11):
        parts = G.split_dataset(data, n)
        assert parts == PR.split_dataset(data, n) and len(parts) == n and sum(parts, []) == data
        assert all(len(p) == len(data) // n for p in parts[:-1])


def test_voc_xml_and_coco_split_line():
    from weclip_vit_comer_amd.clip import generate_cams as G
    names = ["aeroplane", "bird", "cat"]
    new_names = ["aeroplane", "bird avian", "cat"]
    xml = ("<annotation><size><width>500</width><height>375</height><depth>3</depth></size>"
           "<object><name>cat</name></object><object><name>bird</name></object><object><name>cat</name></object></annotation>")
    assert G.voc_label_ids(xml, names, new_names) == ([2, 1], (375, 500))
    assert G.voc_label_ids("<annotation><size><width>4</width><height>3</height></size></annotation>", names, new_names) == ([], (3, 4))
    assert G.coco_split_line("COCO_train2014_000000000009 45 49 50\n") == ("COCO_train2014_000000000009", [45, 49, 50])
    assert G.coco_split_line("x") == ("x", [])


def test_dropin_names_resolve_to_this_package():
    code = ("import weclip_vit_comer_amd as P; P.install_dropin(); import clip.generate_cams_voc12 as v, clip.generate_cams_coco14 as c; "
            "import weclip_vit_comer_amd.clip.generate_cams_voc12 as rv; assert v is rv, v; "
            "assert c.__name__.startswith('weclip_vit_comer_amd'); assert v.BOX_THRESHOLD == 0.4 and c.BOX_THRESHOLD == 0.7; "
            "a = v.parse_args(['--img_root', 'i', '--model', 'm', '--num_workers', '3']); assert a.num_workers == 3; print('ok')")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=root)
    assert r.returncode == 0 and "ok" in r.stdout, r.stderr


def test_new_abi_symbols_exist_and_refuse_bad_arguments():
    import ctypes
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib = _lib.lib()
    for name in ("wc_clip_preprocess", "wc_clip_preprocess_workspace_bytes", "wc_cam_scale_resize_f16", "wc_cam_resize_f32"):
        assert hasattr(lib.cdll, name)
    n = ctypes.c_long(0)
    lib.wc_clip_preprocess_workspace_bytes(2, 375, 500, 384, 512, ctypes.byref(n))
    assert n.value == 2 * 512 * 36 * 4 + 2 * 375 * 512 * 3
    with pytest.raises(RuntimeError, match="down-scaling"):
        lib.wc_clip_preprocess_workspace_bytes(1, 1024, 64, 64, 64, ctypes.byref(n))
    with pytest.raises(RuntimeError, match="bad argument"):
        lib.wc_clip_preprocess(None, None, None, None, None, 0, 1, 8, 8, 16, 16, None, None, None)
    f3 = (ctypes.c_float * 3)(1, 1, 1)
    p16 = ctypes.c_void_p(16)
    with pytest.raises(RuntimeError, match="workspace too small"):          # refused on the host, nothing launched
        lib.wc_clip_preprocess(p16, p16, None, None, p16, 2 * 16 * 36 * 4 + 8 * 16 * 3 - 1, 1, 8, 8, 16, 16, f3, f3, None)
    with pytest.raises(RuntimeError, match="token grid"):
        lib.wc_cam_scale_resize_f16(ctypes.c_void_p(16), ctypes.c_void_p(16), ctypes.c_void_p(16), ctypes.c_void_p(16), 10, 1, 128, 128,
                                    10, None)


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")
def test_preprocess_kernels_issue_their_loads_together(tmp_path):
    """tools/isa_scan.py reports nothing for csrc/preprocess.hip: no load waited for on its own."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, "tools"))
    import isa_scan
    rows = isa_scan.report([os.path.join(root, "weclip-vit-comer_amd", "csrc", "preprocess.hip")], threshold=4, out_dir=str(tmp_path))
    assert not rows, "loads waited for one at a time (see tools/isa_scan.py): %s" % [(r[0], r[1], r[3]) for r in rows]


def test_no_cpu_fallback():
    import torch
    from weclip_vit_comer_amd.clip.generate_cams import ClipPreprocess
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(RuntimeError, match="GPU"):
        ClipPreprocess()(torch.zeros(8, 8, 3, dtype=torch.uint8))
