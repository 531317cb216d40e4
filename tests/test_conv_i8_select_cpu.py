"""Which kernel a dense int8 convolution runs on, held on a box without a GPU: csrc/fq_conv_i8_select.h compiled as
host code with the address and undefined-behaviour sanitizers into scripts/conv_i8_select_check.cpp, which prints the whole choice of
every case and exits non-zero on a violated invariant (grid coverage, the XCD-ordered grid, ring depth, the two-workgroups-per-CU LDS
budget, C % 128 and K % TK, linear_wave's plane).  Held here: the kernel names that the GPU tests assert through conv_variant_log
(copies of their expectations), the three chip-filling thresholds one workgroup below, at and above kCUs, the switch settings the
suite runs, every switch's parse, and golden G21 -- the record of what the dispatcher launched for every case of
tests/conv_select_cases.py BEFORE the selector existed (scripts/int8_conv_choice_dump.py against that build)."""
import os
import re
import subprocess

import pytest

import conv_select_cases as cs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pytorch-quantity_amd", "csrc")
KNOBS = ("FQ_CONV_XCD", "FQ_CONV_STAGES", "FQ_CONV_HALO", "FQ_HALO_STAGES", "FQ_HALO_NP", "FQ_HALO8", "FQ_CONV_C64_HALO", "FQ_C64_XCD",
         "FQ_C64_WG_PER_CU", "FQ_LINEAR_WAVE", "FQ_CONV_DMA", "FQ_CONV_TK", "FQ_CONV_C64")
FIELDS = ("xcd", "stages", "halo", "halo_stages", "halo_np", "halo8", "c64_halo", "c64_xcd", "c64_wg_per_cu", "linear_wave", "dma", "tk",
          "c64")                                                     # ConvSwitches, in KNOBS' order
ROW = re.compile(r"case (\S+): (\w+/\d+) family (\d+) path (\d) stages (\d) np (\d) out (\d+) grid (\d+),(\d+) block (\d+) lds (\d+) "
                 r"xcd_kt (\d+) tiles_m (\d+) slab (\d+) pixels (\d+) tiles (\d+) chunk (\d+)(?: \| refused: (\w+/\d+))?$")


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("conv_select") / "conv_i8_select_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                           os.path.join(ROOT, "scripts", "conv_i8_select_check.cpp")])

    def run(switches, cases):
        """(the parsed switches, {case: row}) -- row: the kernel, then the fields of the printed choice by name"""
        out = subprocess.run([exe] + list(switches) + list(cases), capture_output=True, text=True)
        lines = out.stdout.splitlines()
        assert out.returncode == 0 and not out.stderr and lines[-1] == "ok, %d cases" % len(cases), out.stdout + out.stderr
        sw = dict(zip(lines[0].split()[1::2], (int(v) for v in lines[0].split()[2::2])))
        assert lines[0].startswith("switches: ") and tuple(sw) == FIELDS
        rows = {}
        for ln in lines[1:-1]:
            m = ROW.match(ln)
            assert m, ln
            names = ("kernel", "family", "path", "stages", "np", "out", "gx", "gy", "block", "lds", "xcd_kt", "tiles_m", "slab", "pixels",
                     "tiles", "chunk")
            rows[m.group(1)] = dict(zip(names, [m.group(2)] + [int(v) for v in m.groups()[2:17]]), refused=m.group(18))
        assert list(rows) == list(dict.fromkeys(cases))
        return sw, rows
    return run


def kernels(rows, cases):
    return [rows[c]["kernel"] for c in cases]


# ---------------------------------------------------------------- 1. what only a GPU asserted
def test_the_gpu_tests_kernel_expectations_hold_on_the_host(check):
    _, rows = check((), [c for c, _ in cs.RES_EXPECT + cs.LINEAR_EXPECT] + [cs.NOT_LINEAR])
    for c, want in cs.RES_EXPECT + cs.LINEAR_EXPECT:
        assert rows[c]["kernel"] == want, c
    assert not rows[cs.NOT_LINEAR]["kernel"].startswith("linear_wave") and rows[cs.NOT_LINEAR]["pixels"] == 0


def test_resnet50s_3x3_layers_at_256_images_and_at_two(check):
    """tests/test_gpu_r50_tables.py at the batch bench.py times: three launches on c64_halo/64, at least 7 on halo8, all 13 stride-1
    layers on the halo kernels, the three stride-2 ones on LDS-DMA; at two images no halo8."""
    big, small = cs.r50_3x3(256), cs.r50_3x3(2)
    _, rows = check((), [c for c, _, _ in big + small])
    count = lambda prefix: sum(n for c, _, n in big if rows[c]["kernel"].startswith(prefix))
    assert count("c64_halo/64") == 3 and count("halo8") >= 7 and count("halo") + count("c64_halo") == 13 and count("dma") == 3
    assert all(rows[c]["kernel"].startswith("dma") == (st == 2) for c, st, _ in big + small)
    assert not any(rows[c]["kernel"].startswith("halo8") for c, _, _ in small)
    assert sum(n for c, st, n in small if st == 1 and rows[c]["kernel"].startswith(("halo/", "c64_halo/"))) == 13


# ---------------------------------------------------------------- 2. the three thresholds
def test_128_row_tiles_start_at_one_workgroup_per_cu(check):
    """wg128 = ceil(M / 128) * ceil(K / 128) < kCUs keeps 64-row tiles: 255 pixel tiles -> TK 64, 256 and 257 -> TK 128."""
    _, rows = check((), cs.TK_1X1 + cs.TK_3X3)
    assert kernels(rows, cs.TK_1X1) == ["tile_c128/64", "tile_c128/128", "tile_c128/128"]
    assert [rows[c]["tiles_m"] for c in cs.TK_1X1] == list(cs.AROUND)
    assert [(rows[c]["gx"], rows[c]["gy"], rows[c]["xcd_kt"]) for c in cs.TK_1X1] == [(512, 1, 2), (256, 1, 0), (257, 1, 0)]
    # the 3x3 layers: at 255 pixel tiles the 64-row form has 128 x 2 = 256 tiles of 256 pixels and fills the chip (halo8); the
    # 128-row form of 256 and 257 pixel tiles has 128 and 129
    assert kernels(rows, cs.TK_3X3) == ["halo8/64", "halo/128", "halo/128"]


def test_the_dma_ring_of_three_ends_above_one_workgroup_per_cu(check):
    """grid.x * grid.y <= kCUs: 3 stages.  By default 255 pixel tiles run 64-row tiles (510 workgroups); FQ_CONV_TK=128 makes the
    three cases 255, 256 and 257 workgroups."""
    _, rows = check((), cs.RING_3X3)
    assert kernels(rows, cs.RING_3X3) == ["dma2/64", "dma3/128", "dma2/128", "dma3/64", "dma2/64"]
    wgs = lambda r: r["tiles_m"] * max(r["xcd_kt"], 1) if r["xcd_kt"] else r["gx"] * r["gy"]
    assert [wgs(rows[c]) for c in cs.RING_3X3] == [510, 256, 257, 256, 258]
    _, forced = check(("FQ_CONV_TK=128",), cs.RING_3X3[:3])
    assert kernels(forced, cs.RING_3X3[:3]) == ["dma3/128", "dma3/128", "dma2/128"]
    assert [(forced[c]["gx"], forced[c]["gy"], forced[c]["stages"]) for c in cs.RING_3X3[:3]] == [(255, 1, 3), (256, 1, 3), (257, 1, 2)]


def test_the_eight_wave_halo_kernel_starts_at_one_workgroup_per_cu(check):
    """ceil(M / 256) * (K / TK) >= kCUs: 255 tiles of 256 pixels stay on the 128-pixel halo kernel, 256 and 257 run halo8."""
    _, rows = check((), cs.HALO8_3X3)
    assert kernels(rows, cs.HALO8_3X3) == ["halo/128", "halo8/128", "halo8/128"]
    assert [(rows[c]["gx"], rows[c]["block"]) for c in cs.HALO8_3X3] == [(510, 256), (256, 512), (257, 512)]
    assert all(rows[c]["lds"] <= 80 * 1024 - 64 - 8 * 128 for c in cs.HALO8_3X3)


def test_a_slab_that_does_not_fit_two_workgroups_per_cu_is_no_halo_launch(check):
    """130 + 2 W rows of 128 bytes beside the weight ring in 80 KB less the static part: W = 128 fits (50 176 + 3 x 8 192 + 640),
    W = 256 (82 944 for the slab alone) does not and runs LDS-DMA: 32 x 2 workgroups, a ring of 3."""
    _, rows = check((), cs.WIDE_3X3)
    assert kernels(rows, cs.WIDE_3X3) == ["halo/64", "dma3/64"]
    assert (rows[cs.WIDE_3X3[0]]["slab"], rows[cs.WIDE_3X3[0]]["stages"], rows[cs.WIDE_3X3[0]]["lds"]) == (392, 3, 75392)


# ---------------------------------------------------------------- 3. the switch settings the suite runs
def test_halo8_everywhere_with_and_without_a_ring_of_three(check):
    wide, c64 = cs.HALO_SMALL[:4], cs.HALO_SMALL[4:]                  # C % 128 == 0; C == 64 and K <= 64
    for switches, stages in ((("FQ_HALO8=2",), 2), (("FQ_HALO8=2", "FQ_HALO_STAGES=3"), 3)):
        _, rows = check(switches, cs.HALO_SMALL)
        assert all(rows[c]["kernel"].startswith("halo8/") and rows[c]["stages"] == stages and rows[c]["block"] == 512 for c in wide)
        assert all(rows[c]["kernel"] == "c64_halo/64" for c in c64)
        assert all(rows[c]["refused"].startswith(("dma", "tile_c64")) for c in cs.HALO_SMALL)
    _, rows = check((), cs.HALO_SMALL)
    assert all(rows[c]["kernel"].startswith("halo/") and rows[c]["np"] == 1 for c in wide)
    _, rows = check(("FQ_HALO_NP=2",), wide)
    assert all(rows[c]["kernel"].startswith("halo/") and rows[c]["np"] == 2 for c in wide)


def test_forced_128_row_tiles_with_and_without_a_ring_of_two(check):
    cases = cs.DEEP_SMALL + cs.SHALLOW_SMALL + cs.HALO_SMALL[:2]
    _, rows = check(("FQ_CONV_TK=128",), cases)
    assert all(rows[c]["kernel"].endswith("/128") for c in cases)
    assert kernels(rows, cs.DEEP_SMALL) == ["dma3/128"] * 5 and kernels(rows, cs.HALO_SMALL[:2]) == ["halo/128"] * 2
    assert kernels(rows, cs.SHALLOW_SMALL) == ["tile_c128/128", "tile_c64/128", "tile_c64/128", "tile_general/128", "tile_c64/128"]
    _, rows = check(("FQ_CONV_TK=128", "FQ_CONV_STAGES=2"), cs.DEEP_SMALL)
    assert kernels(rows, cs.DEEP_SMALL) == ["dma2/128"] * 5
    _, rows = check((), cs.DEEP_SMALL)
    assert kernels(rows, cs.DEEP_SMALL) == ["dma3/64"] * 5


def test_without_lds_dma_the_deep_layers_run_the_register_staged_kernel(check):
    cases = cs.HALO_SMALL[:4] + cs.DEEP_SMALL
    _, rows = check(("FQ_CONV_DMA=0",), cases)
    assert kernels(rows, cases) == ["tile_c128/64"] * len(cases)


def test_a_refused_halo_kernel_falls_to_lds_dma_and_a_refused_c64_to_the_tiles(check):
    """The path no launch can take: ensure_dynamic_lds refusing a kernel.  halo8 falls to LDS-DMA, not to the 128-pixel halo."""
    _, rows = check((), cs.HALO8_3X3 + cs.HALO_SMALL)
    assert [rows[c]["refused"] for c in cs.HALO8_3X3] == ["dma2/128"] * 3
    assert [rows[c]["refused"] for c in cs.HALO_SMALL] == ["dma3/64"] * 4 + ["tile_c64/64"] * 2
    _, rows = check((), cs.DEEP_SMALL)
    assert all(rows[c]["refused"] is None for c in cs.DEEP_SMALL)


def test_every_switch_parses_as_it_always_did(check):
    """unset; the empty string (on for the on/off switches and FQ_CONV_DMA, 0 for the numbers); "0"; and the values in use."""
    unset, _ = check((), [])
    assert unset == dict(xcd=1, stages=0, halo=1, halo_stages=0, halo_np=0, halo8=1, c64_halo=1, c64_xcd=1, c64_wg_per_cu=2, linear_wave=1,
                         dma=-1, tk=0, c64=1)
    empty, _ = check([k + "=" for k in KNOBS], [])
    assert empty == dict(xcd=1, stages=0, halo=1, halo_stages=0, halo_np=0, halo8=0, c64_halo=1, c64_xcd=1, c64_wg_per_cu=0, linear_wave=1,
                         dma=1, tk=0, c64=1)
    zero, _ = check([k + "=0" for k in KNOBS], [])
    assert zero == dict.fromkeys(FIELDS, 0)
    for knob, field in zip(KNOBS, FIELDS):
        one, _ = check([knob + "=" + v for v in ("0",)], [])
        assert one == dict(unset, **{field: 0}), knob                            # one switch moves one field
    number = {"stages", "halo_stages", "halo_np", "halo8", "c64_wg_per_cu", "tk"}
    for value in ("1", "2", "3", "64", "128"):
        got, _ = check([k + "=" + value for k in KNOBS], [])
        assert got == {f: (int(value) if f in number else 1) for f in FIELDS}, value


# ---------------------------------------------------------------- 4. golden G21
def test_g21_the_selector_names_the_kernel_the_parent_launched(check, golden_dir):
    want = open(os.path.join(golden_dir, "g21_int8_conv_choice.txt")).read().splitlines()
    got = []
    for name, switches, cases in cs.SETTINGS:
        _, rows = check(switches, cases)
        got += ["%s | %s: %s" % (name, c, rows[c]["kernel"]) for c in cases]
    assert len(want) == len(got) >= 60
    for w, g in zip(want, got):
        assert w == g
    assert {ln.split(": ")[1].split("/")[0] for ln in want} == {"c64_halo", "halo8", "halo", "dma2", "dma3", "tile_c128", "tile_c64",
                                                                "tile_general", "linear_wave"}


# ---------------------------------------------------------------- 5. the shape of the source
def test_one_getenv_site_no_launch_macro_and_the_header_needs_no_hip():
    src = open(os.path.join(CSRC, "fq_conv_i8.hip")).read()
    assert len(re.findall(r"\bgetenv\(", src)) == 1 and not re.search(r"#\s*define\s+FQ_(?!WAVES_TK)", src)
    assert len(re.findall(r"note_conv_variant\(", src)) == 1 and "__global__ __launch_bounds__(256) void quantize_i8" not in src
    header = open(os.path.join(CSRC, "fq_conv_i8_select.h")).read()
    assert re.findall(r"#include\s+(\S+)", header) == ["<cstddef>", "<cstdlib>"] and "getenv" not in header.replace("getenv in", "")
    assert all('"%s"' % k in header for k in KNOBS)
    makefile = open(os.path.join(CSRC, "Makefile")).read()
    assert " fq_quantize_i8.hip " in makefile and " fq_conv_i8_select.h " in makefile and "FILEFLAGS_fq_conv_i8 :=" in makefile
