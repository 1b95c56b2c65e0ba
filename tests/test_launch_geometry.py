"""The geometry of a fused launch and of a multi-GPU tile: sobfu_amd/csrc/sobfu_geometry.hpp (planes per march, workgroup counts,
box numbering) and sobfu_amd/csrc/sobfu_tile_layout.hpp (owned cells, halo messages, pass A's push boxes, the slab schedules' plane
ranges), through tests/cpp/geometry_tool.cpp (g++, no GPU).  Like a wrong variant, a wrong chunk length changes no bits -- it is only
slower, or drops a box -- so no parity test can see it; it is pinned here.

Case lines and answers are described at the top of the tool.  Two kinds of expectation:

* LAUNCH PLANS, PUSH BOXES and PLANE RANGES are compared with tests/golden/launch_geometry.tsv (tuning environment, case, answer).  The
  answers were recorded from the functions as they stood in solver_kernels.hip and tiled_capi.hip before the geometry moved into the
  two headers (pick_zc .. fill_tile_boxes, the launchers' lines around them, make_layout, build_a_boxes, the bookkeeping of
  sobfu_hip_tiled_create3 and the plane ranges of tiled_step_impl): their text, cut out of that commit by line ranges and compiled in a
  scratch harness outside the tree with a fake handle and a stub that captures the planned box lists.  They are not derived from the
  code under test.  A case that is missing from the file fails.
* TILE LAYOUTS and the message bookkeeping are compared with sobfu_amd.tiled.TileLayout, the independent Python statement of the same
  layout, computed here.

Two figures quoted in the code's comments are checked as anchors of their own: pass B at 256^3 beyond the cache is 768 workgroups (six
chunks of 43 planes), and pass B of the 2 x 2 x 2 tile of 256^3 is 15 chunks -> 480 + 288 workgroups.

Recorded as it is, not as it should be: finish_boxes stops at kMaxBoxes = 6 live boxes and drops a seventh without a word (the
launchers refuse more than 6 boxes before it is reached)."""
import os
import subprocess

import numpy as np
import pytest

from sobfu_amd.tiled import TileLayout

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "launch_geometry.tsv")
KNOBS = ("SOBFU_ZC_A", "SOBFU_ZC_B", "SOBFU_CACHE_CELLS")
RESIDENT_CELLS = 3300000  # sobfu_variant.hpp, env_cache_cells(): what launch_pass_b derives `resident` from

GRIDS = [((40, 24, 36), (1, 1, 2)), ((40, 24, 36), (1, 1, 3)), ((40, 24, 36), (2, 1, 1)), ((40, 24, 36), (1, 2, 2)), ((40, 24, 36), (2, 2, 2)),
         ((33, 17, 16), (1, 2, 2)), ((70, 33, 23), (2, 1, 1)), ((64, 64, 64), (2, 2, 2)), ((256, 256, 256), (2, 2, 2))]
# push boxes only: a z-slab with wide rows (y / z faces that store at home on an unconnected handle too)
PUSH_GRIDS = GRIDS + [((128, 40, 64), (1, 1, 4))]


def box(x0, x1, y0, y1, z0, z1, direct=0):
    return "%d %d %d %d %d %d %d" % (x0, x1, y0, y1, z0, z1, direct)


def pass_a(dims, boxes):
    return "A %d %d %d %d %s" % (*dims, len(boxes), " ".join(boxes))


def pass_b(dims, boxes, pipe=None):
    """resident / pipe as launch_pass_b derives them for the solver's own format (pipe follows resident); pipe=0: the API format"""
    resident = int(dims[0] * dims[1] * dims[2] <= RESIDENT_CELLS)
    return "B %d %d %d %d %d %d %s" % (*dims, resident, resident if pipe is None else pipe, len(boxes), " ".join(boxes))


def tile_a(dims, boxes):
    return "T %d %d %d %d %s" % (*dims, len(boxes), " ".join(boxes))


def tile_b_boxes(lay, za, zb, za2=0, zb2=0, shells=True):
    """the six boxes of the tiled loop's pass B launch (pass_b in tiled_capi.hip): two plane ranges of the owned block, the y and x shells"""
    ax0, ax1, ay0, ay1, lo, hi = lay.own_box()
    return [box(ax0, ax1, ay0, ay1, za, zb), box(ax0, ax1, ay0, ay1, za2, zb2),
            box(ax0, ax1, ay0 - 1, ay0 if shells and lay.lo3[1] else ay0 - 1, lo, hi, 1), box(ax0, ax1, ay1, ay1 + 1 if shells and lay.hi3[1] else ay1, lo, hi, 1),
            box(ax0 - 1, ax0 if shells and lay.lo3[0] else ax0 - 1, ay0, ay1, lo, hi, 1), box(ax1, ax1 + 1 if shells and lay.hi3[0] else ax1, ay0, ay1, lo, hi, 1)]


def message_boxes(lay, with_own=True):
    """a tile's pass A list as a connected handle plans it, without the faces that store at home: one direct or marching push box per
    message (fake destinations), then the owned block"""
    out = []
    for i, (peer, sb, rb) in enumerate(lay.messages()):
        march = sb[1] - sb[0] >= 64
        out.append("%s %d %d %d %d %d %d %d %d 0 0" % (box(*sb, 0 if march else 1), 4096 * (i + 1), 1, 2, 3, lay.L[0], lay.L[1], sb[2], sb[3]))
    if with_own:
        out.append(box(*lay.own_box()) + " 0 0 0 0 0 0 0 0 0 0")
    return out


def plan_cases():
    cases = {"": []}
    c = cases[""]
    for n in (64, 128, 256, 512):  # whole grids, both passes; pass B in the solver's format and in the API format
        c += [pass_a((n, n, n), [box(0, n, 0, n, 0, n)]), pass_b((n, n, n), [box(0, n, 0, n, 0, n)]), pass_b((n, n, n), [box(0, n, 0, n, 0, n)], pipe=0)]
    odd = (70, 33, 80)
    c += [pass_a(odd, [box(0, 70, 0, 33, 0, 80)]), pass_b(odd, [box(0, 70, 0, 33, 0, 80)]), pass_b(odd, [box(0, 70, 0, 33, 0, 80)], pipe=0)]
    g64 = (64, 64, 64)
    for planes in (1, 2):  # a box of one plane, of two planes
        c += [pass_a(g64, [box(0, 64, 0, 64, 5, 5 + planes)]), pass_b(g64, [box(0, 64, 0, 64, 5, 5 + planes)]), pass_b(g64, [box(0, 64, 0, 64, 5, 5 + planes)], pipe=0)]
    hole = [box(0, 64, 0, 64, 0, 20), box(0, 64, 10, 10, 20, 40), box(0, 64, 0, 64, 40, 64)]  # an empty box inside a list
    c += [pass_a(g64, hole), pass_b(g64, hole), pass_a(g64, [box(0, 0, 0, 0, 0, 0)]), pass_b(g64, [box(0, 0, 0, 0, 0, 0)])]
    # the two plane ranges of an overlapped slab launch: an interior slab of 1 x 1 x 8 over 256^3 (local planes [4, 36) of 40)
    slab = TileLayout((256, 256, 256), (1, 1, 8), 3)
    sd = slab.L
    c += [pass_a(sd, [box(0, 256, 0, 256, 4, 8), box(0, 256, 0, 256, 32, 36)]), pass_a(sd, [box(0, 256, 0, 256, 8, 32), box(0, 256, 0, 256, 0, 0)]),
          pass_b(sd, tile_b_boxes(slab, 7, 33)), pass_b(sd, tile_b_boxes(slab, 3, 7, 33, 37))]
    # pass B of the 132^3 tiles of a 2 x 2 x 2 split of 256^3 with their thin shells: the even split, rem > 0, the reserve, pair
    for rank in (0, 7):
        t = TileLayout((256, 256, 256), (2, 2, 2), rank)
        z0, z1 = t.o0[2] - (1 if t.lo3[2] else 0), t.o1[2] + (1 if t.hi3[2] else 0)
        c += [pass_b(t.L, tile_b_boxes(t, z0, z1)), pass_b(t.L, tile_b_boxes(t, z0, z1, shells=False)), pass_a(t.L, [box(*t.own_box())])]
    # thin boxes: spread on (pass B) and off (pass A, which takes the tile kernel's list)
    thin = [box(4, 5, 4, 132, 4, 132, 1), box(4, 132, 131, 132, 4, 132, 1), box(4, 20, 4, 8, 4, 132, 1)]
    c += [pass_b((136, 136, 136), [box(4, 132, 4, 132, 3, 133)] + thin), pass_a((136, 136, 136), [box(4, 132, 4, 132, 4, 132)] + thin),
          pass_a((136, 136, 136), thin), pass_b((136, 136, 136), thin), pass_a((256, 256, 256), [box(0, 256, 0, 256, 0, 256), box(0, 3, 0, 256, 0, 256, 1)])]
    # a tile's pass A: 18 push boxes plus the owned block (the centre tile of 3 x 3 x 3), thin rows and wide rows, resident and not
    for dims in ((96, 96, 96), (256, 96, 96), (768, 480, 480)):
        t = TileLayout(dims, (3, 3, 3), 13)
        c += [tile_a(t.L, message_boxes(t)), tile_a(t.L, message_boxes(t, with_own=False))]
    t = TileLayout((96, 96, 96), (3, 3, 3), 13)
    c.append(tile_a(t.L, message_boxes(t) + message_boxes(t)[:2]))  # 21 boxes: refused
    c.append(tile_a(t.L, message_boxes(t) + [box(0, 0, 0, 0, 0, 0) + " 0 0 0 0 0 0 0 0 0 0"] * 3))  # 19 live ones and empty ones: not refused
    # seven live boxes: finish_boxes keeps six
    seven = [box(0, 64, 0, 64, 8 * i, 8 * i + 8) for i in range(7)]
    c += [pass_a(g64, seven), pass_b(g64, seven), pass_b(g64, seven[:5] + [box(0, 1, 0, 64, 0, 64, 1), box(0, 64, 0, 1, 0, 64, 1)])]
    # tuning overrides: planes per march below and above nz
    whole = [pass_a((128, 128, 128), [box(0, 128, 0, 128, 0, 128)]), pass_b((128, 128, 128), [box(0, 128, 0, 128, 0, 128)]),
             pass_b((256, 256, 256), [box(0, 256, 0, 256, 0, 256)]), pass_a(g64, hole), pass_b(g64, hole),
             pass_a((136, 136, 136), [box(4, 132, 4, 132, 4, 132)] + thin), tile_a(t.L, message_boxes(t))]
    for env in ("SOBFU_ZC_A=3", "SOBFU_ZC_A=1000", "SOBFU_ZC_B=3", "SOBFU_ZC_B=1000", "SOBFU_ZC_A=16 SOBFU_ZC_B=16", "SOBFU_CACHE_CELLS=0"):
        cases[env] = list(whole)
    return {env: list(dict.fromkeys(lines)) for env, lines in cases.items()}  # (a size beyond the cache has pipe = 0 either way)


def push_cases():
    out = []
    for dims, grid in PUSH_GRIDS:
        for rank in range(grid[0] * grid[1] * grid[2]):
            out += ["P %d %d %d %d %d %d %d %d 0" % (*dims, *grid, rank, connected) for connected in (0, 1)]
    for skip in (128, 256, 512):  # the timing experiments' switches
        out.append("P 256 256 256 2 2 2 5 1 %d" % skip)
    return out


@pytest.fixture(scope="module")
def tool():
    from sobfu_amd import build_host

    return build_host.build_geometry_tool()


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return {(env, case): answer for env, case, answer in (line.rstrip("\n").split("\t") for line in f if line.strip())}


def run(tool, env, lines):
    e = {k: v for k, v in os.environ.items() if k not in KNOBS}
    e.update(kv.split("=") for kv in env.split())
    r = subprocess.run([tool], input="\n".join(lines) + "\n", capture_output=True, text=True, env=e, timeout=60, check=True)
    out = r.stdout.splitlines()
    assert len(out) == len(lines)
    return out


@pytest.mark.parametrize("env", list(plan_cases()))
def test_launch_plans_are_the_recorded_ones(tool, golden, env):
    lines = plan_cases()[env]
    got = run(tool, env, lines)
    assert list(zip(lines, got)) == [(c, golden.get((env, c), "not recorded")) for c in lines]


def test_push_boxes_and_plane_ranges_are_the_recorded_ones(tool, golden):
    lines = push_cases()
    got = run(tool, "", lines)
    assert list(zip(lines, got)) == [(c, golden.get(("", c), "not recorded")) for c in lines]


def test_quoted_workgroup_counts(tool):
    n = 256
    got = run(tool, "", [pass_b((n, n, n), [box(0, n, 0, n, 0, n)])])[0].split(" | ")
    assert got[0].split()[:2] == ["groups", "768"]  # 128 tiles x 6 chunks ...
    assert got[2].split()[6] == "43"                # ... of 43 planes (pick_zc, capacity 768, refill 6)
    t = TileLayout((n, n, n), (2, 2, 2), 0)
    got = run(tool, "", [pass_b(t.L, tile_b_boxes(t, 0, 129))])[0].split(" | ")
    head = got[0].split()
    # 32 tiles x 15 chunks of 8 or 9 planes (129 = 15 * 8 + 9), then the y shell (32 workgroups) and the x shell (256 of one wave)
    assert head[:4] == ["groups", "768", "0", "480"] and got[2].split()[6:11] == ["8", "0", "8", "9", "1"]
    assert [int(v) for v in head[5:12]] == [0, 480, 512, 768, 768, 768, 768]


def expected_layout(dims, grid, rank):
    """the tool's answer to an L case, from TileLayout"""
    t = TileLayout(dims, grid, rank)
    s = "P %d %d %d c %d %d %d" % (*grid, *t.coords)
    for a in range(3):
        s += " | %d %d %d %d %d %d %d %d" % (t.g0[a], t.g1[a], t.lo3[a], t.hi3[a], t.L[a], t.o0[a], t.o1[a], t.base[a])
    msgs = t.messages()
    cells = [(sb[1] - sb[0]) * (sb[3] - sb[2]) * (sb[5] - sb[4]) for _, sb, _ in msgs]
    z_face = [sb[0:4] == rb[0:4] == (t.o0[0], t.o1[0], t.o0[1], t.o1[1]) for _, sb, rb in msgs]  # x and y ranges are the owned ones
    assert z_face == sorted(z_face)  # z faces last
    n_packed = len(msgs) if t.slab else z_face.count(False)
    s += " | msgs %d packed %d floats %d" % (len(msgs), n_packed, 3 * sum(cells))
    off = 0
    for (peer, sb, rb), n in zip(msgs, cells):  # packed one after the other, the same offsets on both sides
        s += " | %d %s %s %d %d %d %d" % (peer, " ".join(map(str, sb)), " ".join(map(str, rb)), peer, off, off, 3 * n)
        off += 3 * n
    plane = t.L[0] * t.L[1] * 3
    inplace = [] if t.slab else [(peer, plane * sb[4], plane * rb[4], plane * t.halo) for (peer, sb, rb), zf in zip(msgs, z_face) if zf]
    s += " | inplace %d" % len(inplace) + "".join(" | %d %d %d %d" % m for m in inplace)
    tab = []
    for _, _, rb in ([] if t.slab else msgs[:n_packed]):  # x fastest inside a message's box
        z, y, x = np.meshgrid(np.arange(rb[4], rb[5]), np.arange(rb[2], rb[3]), np.arange(rb[0], rb[1]), indexing="ij")
        tab.append((x + t.L[0] * (y + t.L[1] * z)).ravel())
    tab = np.concatenate(tab).astype(np.uint64) if tab else np.zeros(0, np.uint64)
    with np.errstate(over="ignore"):
        h = int(np.sum(np.arange(1, tab.size + 1, dtype=np.uint64) * tab, dtype=np.uint64))
    return s + " | scatter %d %d" % (tab.size, h)


@pytest.mark.parametrize("dims,grid", GRIDS)
def test_layout_is_the_python_layout(tool, dims, grid):
    ranks = range(grid[0] * grid[1] * grid[2])
    got = run(tool, "", ["L %d %d %d %d %d %d %d" % (*dims, *grid, r) for r in ranks])
    assert got == [expected_layout(dims, grid, r) for r in ranks]


def test_thin_tiles_are_refused(tool):
    assert run(tool, "", ["L 6 12 12 2 1 1 0", "L 6 12 12 2 1 1 1", "P 12 7 12 1 2 1 0 0 0", "L 12 12 8 1 1 2 0"])[:3] == ["refused"] * 3
    with pytest.raises(ValueError):
        TileLayout((6, 12, 12), (2, 1, 1), 0)
