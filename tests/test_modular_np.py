"""The Modular sample decode and its transforms held to the reading of tests/modular_np.py on the CPU: both front-ends --
the product's (libjxl_amd/csrc/host/jxh_modular.h) and the oracle's (oracle/jxlo_modular.h), each compiled into its own
copy of tests/c/modular_model_kats.cc with AddressSanitizer + UBSan -- decode the bytes the reading's writer made and must
return the reading's channels exactly, before the transforms are undone and after. That holds their parse of the group
header, the weighted-predictor header, the transform list and the tree as well. The reading is checked against itself (its
writer's bytes come back through tests/ans_np.py's reader and reconstruct()), every named misreading is shown to change a
case, and flipped bits must end as an error of the program or a decode, never as a sanitizer report.

The cases are those of tests/modular_cases.py; tests/test_gpu_modular_np.py runs the same ones through the kernels."""
import os
import random
import subprocess

import pytest

import modular_cases as C
import modular_np as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    d = tmp_path_factory.mktemp("modular_model_kats")
    out = {}
    for which in ("product", "oracle"):
        out[which] = str(d / which)
        subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall",
                        "-Wno-unused-function"] + (["-DKAT_ORACLE"] if which == "oracle" else []) +
                       [os.path.join(ROOT, "tests", "c", "modular_model_kats.cc"), "-o", out[which]], check=True)
    return out


def case_file(case, path):
    data = case.stream["data"]
    with open(path, "w") as f:
        f.write("%d %d %d %d %d\n" % (len(case.shapes), case.nb_meta, case.stream_id, case.bit_depth, len(data)))
        for s in case.shapes:
            f.write("%d %d %d %d\n" % s)
        f.write(data.hex() + "\n")
    return str(path)


def parse_output(text):
    """-> {"pre": (end_bit, nb_meta, [(shape, samples)]), "final": ...}"""
    lines = text.splitlines()
    out, i = {}, 0
    while i < len(lines):
        end_bit = int(lines[i].split()[1])
        name, n, nb_meta = lines[i + 1].split()
        chans = []
        for ln in lines[i + 2:i + 2 + int(n)]:
            v = [int(t) for t in ln.split()]
            chans.append((tuple(v[:4]), v[4:]))
        out[name] = (end_bit, int(nb_meta), chans)
        i += 2 + int(n)
    return out


def as_listed(chans):
    return [(c.shape(), c.flat()) for c in chans]


@pytest.mark.parametrize("name", C.NAMES)
def test_the_writers_bytes_come_back_through_the_plain_reader(name):
    """ans_np.Reader from the bit position the writer reported, and reconstruct(): the samples, the coder's final state and
    the end of the stream."""
    case = C.build(name)
    chans, reader = M.read_back(case.stream, [c.shape() for c in case.pre], case.tree, case.wp_values, case.stream_id)
    assert as_listed(chans) == as_listed(case.pre)
    assert reader.final_state_ok() and reader.pos == case.stream["end_bit"]
    assert case.stream["end_bit"] <= len(case.stream["data"]) * 8 < case.stream["end_bit"] + 8


@pytest.mark.parametrize("which", ["product", "oracle"])
@pytest.mark.parametrize("name", C.NAMES)
def test_front_end_returns_the_readings_channels(programs, tmp_path, which, name):
    case = C.build(name)
    r = subprocess.run([programs[which], case_file(case, tmp_path / "case.txt")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-400:] + r.stderr[-2000:]
    got = parse_output(r.stdout)
    end_bit, nb_meta, chans = got["pre"]
    assert (end_bit, nb_meta) == (case.stream["end_bit"], case.pre_nb_meta)
    assert chans == as_listed(case.pre), "before the transforms are undone"
    end_bit, nb_meta, chans = got["final"]
    assert (end_bit, nb_meta) == (case.stream["end_bit"], case.nb_meta)
    assert chans == as_listed(case.final), "after the transforms are undone"


def test_the_cases_reach_what_they_are_there_for(monkeypatch):
    for name in ("props", "prev_wp", "rects") + tuple(n for n in C.NAMES if n.startswith("wp_")):
        case = C.build(name)
        assert set(ctx for ctx, _ in case.tokens) == set(range(M.num_leaves(case.tree))), name + ": a leaf no sample reaches"
    props = C.build("props")
    assert sorted(n[0] for n in props.tree if n[0] >= 0) == list(range(2, 16))
    assert (4, -5, 3) in [n[2:] for n in props.tree if n[0] < 0] and 2 << 4 in [n[4] for n in props.tree if n[0] < 0]
    prev = C.build("prev")
    assert sorted(n[0] for n in prev.tree if n[0] >= 0) == list(range(16, 32))
    assert M.reference_channels(prev.pre, 6, 32) == [5, 3, 1, 0]  # nearest first, past the shifted and the smaller one
    assert len(set(ctx for ctx, _ in prev.tokens)) >= 15
    a, b = C.build("static_s3"), C.build("static_s5")
    assert a.tree == b.tree and set(c for c, _ in a.tokens) != set(c for c, _ in b.tokens)
    for header in ("distinct", "north", "weights_0_15"):
        wp = C.WP_HEADERS[header]
        assert wp["p3Cd"] and wp["p3Ce"]
    d = C.WP_HEADERS["distinct"]
    assert len(set([d[f] for f in M.WP_FIELDS] + list(d["w"]))) == 11
    assert set(C.WP_HEADERS["weights_0_15"]["w"]) == {0, 15}
    for name in ("rct_wrap6", "rct_wrap4"):
        case = C.build(name)
        assert max(abs(v) for c in case.final for v in c.flat()) == 1 << 30
        exact = M.copy_channels(case.pre)
        with monkeypatch.context() as m:
            m.setattr(M, "i32", int)  # the same arithmetic without the narrowing
            M.inverse_transforms(exact, 0, case.filled)
        assert as_listed(exact) != as_listed(case.final), name + ": nothing wrapped"
    branches = set()
    line = C.build("squeeze_line")
    M.squeeze_inverse(M.copy_channels(line.pre), 0, line.filled[0][1], branches=branches)
    assert branches == {"equal", "falling", "falling+a", "falling+b", "rising", "rising+a", "rising+b", "neither"}
    idx = C.build("palette_nb1").pre[1].flat()
    assert min(idx) < 0 and max(idx) > 5
    for bits in (8, 12):
        idx = C.build("palette_nb3_%d" % bits).pre[1].flat()
        assert min(idx) < 0 and any(6 <= v < 70 for v in idx) and any(v >= 70 for v in idx) and any(0 <= v < 6 for v in idx)
    steps = C.build("squeeze_default").filled[0][1]
    assert steps[:2] == [(True, False, 1, 2), (False, False, 1, 2)] and len(steps) == 7


def test_forward_and_inverse_transforms_meet():
    r = random.Random(3)
    for rct_type in range(42):
        image = [M.Chan(5, 2, rows=[[r.choice((r.randint(-300, 300), M.I32_MAX, M.I32_MIN, 1 << 30)) for _ in range(5)] for _ in range(2)])
                 for _ in range(3)]
        coded = M.copy_channels(image)
        M.rct_forward(coded, 0, rct_type)
        M.rct_inverse(coded, 0, rct_type)
        assert [c.d for c in coded] == [c.d for c in image], rct_type
    for n in range(1, 14):
        for _ in range(50):
            line = [r.randint(-40, 40) + 5 * i for i in range(n)]
            avg, res = M.squeeze_line(line)
            assert M.unsqueeze_line(avg, res) == line


# misreading -> (case, what is read again under the misreading)
MISREADING_CASES = {
    "prop8_from_current_9": ("props", "samples"),
    "prop9_not_reset": ("props", "samples"),
    "avg0_floor": ("pred3", "samples"),
    "avg123_floor": ("pred10", "samples"),
    "avg4_floor": ("pred13", "samples"),
    "select_tie_other": ("pred4", "samples"),
    "toprightright_to_top": ("pred13", "samples"),
    "vtop_fallback_zero": ("prev", "samples"),
    "refs_farthest_first": ("prev", "samples"),
    "refs_ignore_shift": ("prev", "samples"),
    "branch_ge": ("props", "samples"),
    "multiplier_on_prediction": ("props", "samples"),
    "wp_round_4": ("wp_default_leaf", "samples"),
    "wp_clamp_always": ("wp_default_leaf", "samples"),
    "wp_no_above_right": ("wp_default_leaf", "samples"),
    "wp_ne_last_zero": ("wp_default_leaf", "samples"),
    "wp_max_error_tie_later": ("wp_default_prop15_only", "samples"),
    "wp_swap_p3d_p3e": ("wp_distinct_leaf", "samples"),
    "rct_swap_permutation_23": ("rct_perm1", "transforms"),
    "rct_avg_truncates": ("rct_perm0", "transforms"),
    "squeeze_diff_floor": ("squeeze_line", "transforms"),
    "squeeze_limit_a": ("squeeze_line", "transforms"),
    "squeeze_limit_b": ("squeeze_line", "transforms"),
    "squeeze_odd_from_residual": ("squeeze_17x9", "transforms"),
    "palette_no_clamp": ("palette_nb1", "transforms"),
    "palette_delta_parity": ("palette_nb3_8", "transforms"),
}


def test_every_misreading_has_a_case():
    assert set(MISREADING_CASES) == set(M.MISREADINGS) and len(M.MISREADINGS) >= 20


@pytest.mark.parametrize("mis", M.MISREADINGS)
def test_misreading_changes_its_case(mis):
    """The case's own token values (or channels) read under the misreading give other samples: a decoder that read the
    rule that way fails test_front_end_returns_the_readings_channels on this case."""
    name, what = MISREADING_CASES[mis]
    case = C.build(name)
    if what == "samples":
        values = [v for _, v in case.tokens]
        shapes = [c.shape() for c in case.pre]
        assert as_listed(M.reconstruct(values, shapes, case.tree, case.wp_values, case.stream_id)) == as_listed(case.pre)
        assert as_listed(M.reconstruct(values, shapes, case.tree, case.wp_values, case.stream_id, mis=[mis])) != as_listed(case.pre)
    else:
        chans = M.copy_channels(case.pre)
        M.inverse_transforms(chans, case.pre_nb_meta, case.filled, case.wp_values, case.bit_depth, mis=[mis])
        assert as_listed(chans) != as_listed(case.final)
    if mis == "avg123_floor":
        for other in ("pred11", "pred12"):
            c = C.build(other)
            got = M.reconstruct([v for _, v in c.tokens], [x.shape() for x in c.pre], c.tree, mis=[mis])
            assert as_listed(got) != as_listed(c.pre), other


@pytest.mark.parametrize("which", ["product", "oracle"])
def test_flipped_bits_end_as_an_error_or_a_decode(programs, tmp_path, which):
    """200 one-bit flips over three cases, header, tree, histograms and samples alike: the program answers every one (an
    error message or a decode) and the sanitizers report nothing."""
    r = random.Random(200)
    seen = {"ok": 0, "error": 0}
    for name, count in (("props", 67), ("squeeze_default", 67), ("palette_rct", 66)):
        case = C.build(name)
        nbits = len(case.stream["data"]) * 8
        head = min(nbits, 400)  # the group header, the transforms and the tree sit here: half of the flips
        bits = r.sample(range(head), min(head, count // 2))
        bits += r.sample(range(nbits), count - len(bits))
        p = subprocess.run([programs[which], case_file(case, tmp_path / (name + ".txt")), "flip"] + [str(b) for b in bits],
                           capture_output=True, text=True, timeout=300)
        assert p.returncode == 0, p.stdout[-300:] + p.stderr[-3000:]
        answers = [ln.split()[:2] for ln in p.stdout.splitlines() if not ln.startswith("end_bit")]
        assert [int(a[0]) for a in answers] == bits
        for a in answers:
            seen[a[1]] += 1
    assert seen["ok"] + seen["error"] == 200 and seen["error"] > 20


def test_descriptor_mirrors_match_the_header(tmp_path):
    """tests/modular_desc.py mirrors the structs of include/jxl_amd_hip.h for the GPU test's hand-made descriptors: a
    compiler says the size of each and the offset of every field."""
    import ctypes

    import modular_desc as D
    lines = ['#include <stddef.h>', '#include <stdio.h>', '#include "jxl_amd_hip.h"', "int main() {"]
    for name, cls in D.MIRRORS.items():
        lines.append('  printf("%s %%zu\\n", sizeof(%s));' % (name, name))
        for field, _ in cls._fields_:
            lines.append('  printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (name, field, name, field))
    lines += ["  return 0;", "}"]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines) + "\n")
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "layout")], check=True)
    said = dict(ln.split() for ln in subprocess.run([str(tmp_path / "layout")], capture_output=True, text=True, check=True).stdout.splitlines())
    for name, cls in D.MIRRORS.items():
        assert int(said[name]) == ctypes.sizeof(cls), name
        for field, _ in cls._fields_:
            assert int(said["%s.%s" % (name, field)]) == getattr(cls, field).offset, (name, field)


def test_hand_made_descriptors_describe_every_gpu_case(tmp_path):
    """The frames of the GPU test are built here too, without a device: every channel of every case finds its place, the
    weighted predictor's scratch is sized by the widest channel, and the upload's own rules (tests/c/modular_desc_check.cc
    over jxh_modular_upload_plan.h) take the descriptor."""
    import ctypes

    import modular_desc as D
    f = D.Frame()
    for k, name in enumerate(C.GPU_NAMES):
        f.add(C.build(name), placed=k % 2 == 1)
    d, keep = f.descriptor()
    assert d.num_streams == len(C.GPU_NAMES) and d.num_trees == d.num_codes == len(C.GPU_NAMES) and d.num_ops == len(f.ops) > 60
    for s in f.streams:
        rects = f.rects[s["first_rect"]:s["first_rect"] + s["num_rects"]]
        assert s["max_width"] == max(r[3] for r in rects) and 16 <= s["num_props"] <= 32
    for buffer, x0, y0, w, h, _ in f.rects:
        assert x0 + w <= f.buffers[buffer][0] and y0 + h <= f.buffers[buffer][1]
    assert any(r[1] == 1 for r in f.rects) and any(r[1] == 3 for r in f.rects) and any(r[3] == 0 for r in f.rects)
    so = str(tmp_path / "modular_desc_check.so")
    subprocess.run(["g++", "-std=c++17", "-O1", "-shared", "-fPIC", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "c", "modular_desc_check.cc"), "-o", so], check=True)
    check = ctypes.CDLL(so).modular_desc_check
    check.argtypes = [ctypes.c_void_p]
    assert check(ctypes.byref(d)) == 0
    d.rects = ctypes.addressof((D.Rect * len(f.rects))(*[D.Rect(r[0], r[1] + 40, *r[2:]) for r in f.rects]))
    assert check(ctypes.byref(d)) == 1000 + 11  # kModRuleRectInsideBuffer: the check does look
