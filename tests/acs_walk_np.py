"""An independent numpy-float32 reading of the merge walk of libjxl's AC-strategy search, lib/jxl/enc_ac_strategy.cc:
TryMergeAcs :618-653, SetEntropyForTransform :655-665, AcsSquare / AcsVerticalSplit / AcsHorizontalSplit :667-695,
FindBestFirstLevelDivisionForSquare :703-825, ProcessRectACS :827-1059 and the two MultiBlockTransformCrosses*Boundary
functions :302-362, for decoding_speed_tier 0 and DCT as the only 8x8 kind. It shares no code with the product: it is written
on the reference's own names, over one tile of w x h blocks with bx = by = 0 (the reference's bx, by are multiples of 8, so
`% 8`, `& ~7` and the comparisons with the image size read the same on the tile's own coordinates: a coordinate of 8 is
either outside the image or a multiple of 8, and both return false).

walk(estimate, w, h, mul8x8, floating) takes estimate(kind, cx, cy) -> float32, the estimate of the candidate of `kind`
(KINDS below) whose top-left block is (cx, cy), with the kind's multiplier already in it. It returns a Walk: .strategy
[8][8] (AcStrategy numbers), .first [8][8], .entropy [64] float32, .asked (the set of (kind, cx, cy) it asked for) and .took
(the names of the branches it went through).

Two stated deviations from the text, shared with the product. They cannot refuse anything on a table of
finite estimates above zero, and make the result a valid tiling on any table: TryMergeAcs makes the four crossing tests of
the square function before it accepts (the reference tries DCT32X64 at (0, 4) of a full tile after the 64-level square, whose
placements carry no priority), and the square function places a half only if it took its estimate (the FLT_MAX that stands
for "not taken" is below an infinite sum). misread="reference_unguarded" is the text as written.

Deliberate misreadings, by name (MISREADINGS): each is a way to read the text wrongly that changes some output.
Left out because it cannot change any output with this merge table: `priority >= candidate_priority` read as `>`. Only
DCT64X32 (both at y 0, disjoint columns) and DCT32X64 meet at one priority; the one DCT32X64 that reaches TryMergeAcs in a
tile that has a DCT64X32 is the one at (0, 4), and over a DCT64X32 it is refused by the crossing tests as well."""
import numpy as np

F = np.float32
FLT_MAX = np.finfo(np.float32).max

# kinds in the order of the estimate table: name, AcStrategy number, covered_blocks_x, covered_blocks_y
KINDS = (("DCT", 0, 1, 1), ("DCT16X8", 6, 1, 2), ("DCT8X16", 7, 2, 1), ("DCT16X16", 4, 2, 2), ("DCT32X16", 10, 2, 4),
         ("DCT16X32", 11, 4, 2), ("DCT32X32", 5, 4, 4), ("DCT64X32", 19, 4, 8), ("DCT32X64", 20, 8, 4), ("DCT64X64", 18, 8, 8))
KIND_OF = {name: i for i, (name, _, _, _) in enumerate(KINDS)}
COVERED = {name: (cx, cy) for name, _, cx, cy in KINDS}
NUMBER = {name: num for name, num, _, _ in KINDS}
MULTIPLIER = {"DCT": 1.0, "DCT16X8": 1.21, "DCT8X16": 1.21, "DCT16X16": 1.34, "DCT32X16": 1.49, "DCT16X32": 1.49, "DCT32X32": 1.48,
              "DCT64X32": 2.25, "DCT32X64": 2.25, "DCT64X64": 2.25}

MISREADINGS = ("no_mul8x8", "no_zeroing", "no_head_checks", "allow_always", "no_64x32_merge", "no_odd_leaks", "le_for_lt",
               "tie_other_way", "floating_swapped", "and_for_or")
UNGUARDED = "reference_unguarded"  # not a misreading: the text without the two guards


def mul8x8(distance):
    return F(1.0) + F(-0.4) / (F(distance) + F(1.4))


class Walk:
    def __init__(self, estimate, w, h, misread):
        self.estimate, self.w, self.h, self.misread = estimate, w, h, misread
        self.type = [["DCT"] * 8 for _ in range(8)]  # the AcStrategyImage of the tile: raw strategy and first-block bit
        self.first = [[True] * 8 for _ in range(8)]
        self.entropy = [F(0)] * 64
        self.priority = [0] * 64
        self.asked, self.took = set(), set()

    @property
    def strategy(self):
        return np.array([[NUMBER[t] for t in row] for row in self.type], np.uint8)

    def ask(self, name, cx, cy):
        self.asked.add((KIND_OF[name], cx, cy))
        return F(self.estimate(KIND_OF[name], cx, cy))

    def set(self, x, y, name):
        cbx, cby = COVERED[name]
        for iy in range(cby):
            for ix in range(cbx):
                self.type[y + iy][x + ix] = name
                self.first[y + iy][x + ix] = (iy | ix) == 0

    # :302-330
    def crosses_horizontal(self, start_x, y, end_x):
        if start_x >= self.w or y >= self.h:
            return False
        if y % 8 == 0:
            return False
        end_x = min(end_x, self.w)
        start_x_limit = start_x & ~7
        while start_x != start_x_limit and not self.first[y][start_x]:
            start_x -= 1
        x = start_x
        while x < end_x:
            if self.first[y][x]:
                x += COVERED[self.type[y][x]][0]
            else:
                return True
        return False

    # :332-362
    def crosses_vertical(self, x, start_y, end_y):
        if x >= self.w or start_y >= self.h:
            return False
        if x % 8 == 0:
            return False
        end_y = min(end_y, self.h)
        start_y_limit = start_y & ~7
        while start_y != start_y_limit and not self.first[start_y][x]:
            start_y -= 1
        y = start_y
        while y < end_y:
            if self.first[y][x]:
                y += COVERED[self.type[y][x]][1]
            else:
                return True
        return False

    def outline_crossed(self, cx, cy, nx, ny):
        return (self.crosses_horizontal(cx, cy, cx + nx) or self.crosses_horizontal(cx, cy + ny, cx + nx) or
                self.crosses_vertical(cx, cy, cy + ny) or self.crosses_vertical(cx + nx, cy, cy + ny))

    # :618-653
    def try_merge(self, name, cx, cy, candidate_priority):
        cbx, cby = COVERED[name]
        entropy_current = F(0)
        for iy in range(cby):
            for ix in range(cbx):
                if self.priority[(cy + iy) * 8 + cx + ix] >= candidate_priority:
                    self.took.add("priority_refused")
                    return
                entropy_current = entropy_current + self.entropy[(cy + iy) * 8 + cx + ix]
        entropy_candidate = self.ask(name, cx, cy)
        if self.misread == "le_for_lt":
            if entropy_candidate > entropy_current:
                return
        elif entropy_candidate >= entropy_current:
            return
        if self.misread != "reference_unguarded" and self.outline_crossed(cx, cy, cbx, cby):
            self.took.add("merge_refused_cut")
            return
        for iy in range(cby):
            for ix in range(cbx):
                if self.misread != "no_zeroing":
                    self.entropy[(cy + iy) * 8 + cx + ix] = F(0)
                self.priority[(cy + iy) * 8 + cx + ix] = candidate_priority
        self.set(cx, cy, name)
        self.entropy[cy * 8 + cx] = entropy_candidate
        self.took.add("merge_" + name)

    # :655-665
    def set_entropy_for_transform(self, cx, cy, name, entropy):
        cbx, cby = COVERED[name]
        if self.misread != "no_zeroing":
            for dy in range(cby):
                for dx in range(cbx):
                    self.entropy[(cy + dy) * 8 + cx + dx] = F(0)
        self.entropy[cy * 8 + cx] = entropy

    # :703-825, allow_square_transform true
    def find_best_first_level_division_for_square(self, blocks, cx, cy, phase):
        blocks_half = blocks // 2
        jxk = {2: "DCT16X8", 4: "DCT32X16", 8: "DCT64X32"}[blocks]  # AcsVerticalSplit
        kxj = {2: "DCT8X16", 4: "DCT16X32", 8: "DCT32X64"}[blocks]  # AcsHorizontalSplit
        jxj = {2: "DCT16X16", 4: "DCT32X32", 8: "DCT64X64"}[blocks]  # AcsSquare
        if self.misread != "no_head_checks" and self.outline_crossed(cx, cy, blocks, blocks):
            self.took.add("head_return")
            return
        allow_jxk = not self.crosses_vertical(cx + blocks_half, cy, cy + blocks)
        allow_kxj = not self.crosses_horizontal(cx, cy + blocks_half, cx + blocks)
        if not allow_jxk:
            self.took.add("allow_JXK_false_" + phase)
        if not allow_kxj:
            self.took.add("allow_KXJ_false_" + phase)
        if self.misread == "allow_always":
            allow_jxk = allow_kxj = True
        entropy = [[F(0), F(0)], [F(0), F(0)]]
        for dy in range(blocks):
            for dx in range(blocks):
                entropy[dy // blocks_half][dx // blocks_half] = entropy[dy // blocks_half][dx // blocks_half] + self.entropy[(cy + dy) * 8 + cx + dx]
        jxk_left = jxk_right = kxj_top = kxj_bottom = FLT_MAX
        taken = set()
        if allow_jxk:
            if self.type[cy][cx] != jxk:
                jxk_left = self.ask(jxk, cx, cy)
                taken.add("left")
            else:
                self.took.add("skip_already_JXK")
            if self.type[cy][cx + blocks_half] != jxk:
                jxk_right = self.ask(jxk, cx + blocks_half, cy)
                taken.add("right")
            else:
                self.took.add("skip_already_JXK")
        if allow_kxj:
            if self.type[cy][cx] != kxj:
                kxj_top = self.ask(kxj, cx, cy)
                taken.add("top")
            else:
                self.took.add("skip_already_KXJ")
            if self.type[cy + blocks_half][cx] != kxj:
                kxj_bottom = self.ask(kxj, cx, cy + blocks_half)
                taken.add("bottom")
            else:
                self.took.add("skip_already_KXJ")
        if self.misread == "reference_unguarded":
            taken = {"left", "right", "top", "bottom"}
        entropy_jxj = self.ask(jxj, cx, cy)
        lt = (lambda a, b: a <= b) if self.misread == "le_for_lt" else (lambda a, b: a < b)
        cost_jxn = min(jxk_left, entropy[0][0] + entropy[1][0]) + min(jxk_right, entropy[0][1] + entropy[1][1])
        cost_nxj = min(kxj_top, entropy[0][0] + entropy[0][1]) + min(kxj_bottom, entropy[1][0] + entropy[1][1])
        jxn_first = cost_jxn <= cost_nxj if self.misread == "tie_other_way" else cost_jxn < cost_nxj
        if lt(entropy_jxj, cost_jxn) and lt(entropy_jxj, cost_nxj):
            self.set(cx, cy, jxj)
            self.set_entropy_for_transform(cx, cy, jxj, entropy_jxj)
            self.took.add("JXJ")
        elif jxn_first:
            self.took.add("JXK_branch")
            if "left" in taken and lt(jxk_left, entropy[0][0] + entropy[1][0]):
                self.set(cx, cy, jxk)
                self.set_entropy_for_transform(cx, cy, jxk, jxk_left)
                self.took.add("JXK_left")
            if "right" in taken and lt(jxk_right, entropy[0][1] + entropy[1][1]):
                self.set(cx + blocks_half, cy, jxk)
                self.set_entropy_for_transform(cx + blocks_half, cy, jxk, jxk_right)
                self.took.add("JXK_right")
        else:
            self.took.add("KXJ_branch")
            if "top" in taken and lt(kxj_top, entropy[0][0] + entropy[0][1]):
                self.set(cx, cy, kxj)
                self.set_entropy_for_transform(cx, cy, kxj, kxj_top)
                self.took.add("KXJ_top")
            if "bottom" in taken and lt(kxj_bottom, entropy[1][0] + entropy[1][1]):
                self.set(cx, cy + blocks_half, kxj)
                self.set_entropy_for_transform(cx, cy + blocks_half, kxj, kxj_bottom)
                self.took.add("KXJ_bottom")

    # :860-1058
    def process_rect_acs(self, mul, floating):
        w, h = self.w, self.h
        for iy in range(h):
            for ix in range(w):
                entropy = self.ask("DCT", ix, iy)
                self.entropy[iy * 8 + ix] = entropy if self.misread == "no_mul8x8" else entropy * F(mul)
        merge = (("DCT16X8", 2), ("DCT8X16", 2), ("DCT16X32", 4), ("DCT32X16", 4), ("DCT64X32", 6), ("DCT32X64", 6))
        for name, priority in merge:
            if self.misread == "no_64x32_merge" and name == "DCT64X32":
                continue
            cbx, cby = COVERED[name]
            for cy in range(0, h, cby):
                if not cy + cby - 1 < h:
                    break
                for cx in range(0, w, cbx):
                    if not cx + cbx - 1 < w:
                        break
                    if cy + 7 < h and cx + 7 < w:
                        if name == "DCT32X64":
                            if (cy | cx) % 8 == 0:
                                self.find_best_first_level_division_for_square(8, cx, cy, "aligned")
                            continue
                        elif name == "DCT32X16":
                            continue
                    if (name == "DCT16X32" and cy % 4 != 0) or (name == "DCT32X16" and cx % 4 != 0):
                        continue
                    if cy + 3 < h and cx + 3 < w:
                        if name == "DCT16X32":
                            if (cy | cx) % 4 == 0:
                                self.find_best_first_level_division_for_square(4, cx, cy, "aligned")
                            continue
                        elif name == "DCT32X16":
                            continue
                    if (name == "DCT16X32" and cy % 4 != 0) or (name == "DCT32X16" and cx % 4 != 0):
                        continue
                    if cy + 1 < h and cx + 1 < w:
                        if name == "DCT8X16":
                            if (cy | cx) % 2 == 0:
                                self.find_best_first_level_division_for_square(2, cx, cy, "aligned")
                            continue
                        elif name == "DCT16X8":
                            continue
                    if (name == "DCT8X16" and cy % 2 == 1) or (name == "DCT16X8" and cx % 2 == 1):
                        continue
                    if self.misread == "no_odd_leaks" and name in ("DCT16X8", "DCT8X16"):
                        continue
                    self.try_merge(name, cx, cy, priority)
        if not floating:
            return

        def pass_16():
            for cy in range(h - 1):
                for cx in range(w - 1):
                    odd = (cy % 2 != 0 and cx % 2 != 0) if self.misread == "and_for_or" else (cy | cx) % 2 != 0
                    if odd:
                        self.find_best_first_level_division_for_square(2, cx, cy, "floating")

        def pass_32():
            for cy in range(h - 3):
                for cx in range(w - 3):
                    if (cy | cx) % 4 == 0:
                        continue
                    self.find_best_first_level_division_for_square(4, cx, cy, "floating")

        for p in ((pass_32, pass_16) if self.misread == "floating_swapped" else (pass_16, pass_32)):
            p()


def walk(estimate, w, h, mul, floating, misread=None):
    assert misread is None or misread in MISREADINGS or misread == UNGUARDED
    wk = Walk(estimate, w, h, misread)
    wk.process_rect_acs(mul, floating)
    return wk


def walk_frame(table, xb, yb, distance, floating, misread=None):
    """The walk over every tile of a frame, on a table [tiles][10][8][8]: (acs [yb][xb] = (strategy << 1) | first, entropy
    [yb][xb] float32, the union of what was asked as (kind, bx, by) in frame coordinates, the union of the branches taken)."""
    table = np.asarray(table, np.float32).reshape(-1, 10, 8, 8)
    tiles_x = (xb + 7) // 8
    acs, ent = np.zeros((yb, xb), np.uint8), np.zeros((yb, xb), np.float32)
    asked, took = set(), set()
    for t in range(table.shape[0]):
        bx0, by0 = (t % tiles_x) * 8, (t // tiles_x) * 8
        w, h = min(8, xb - bx0), min(8, yb - by0)
        wk = walk(lambda k, cx, cy, t=t: table[t, k, cy, cx], w, h, mul8x8(distance), floating, misread)
        acs[by0:by0 + h, bx0:bx0 + w] = (wk.strategy[:h, :w] << 1) | np.array(wk.first, np.uint8)[:h, :w]
        ent[by0:by0 + h, bx0:bx0 + w] = np.array(wk.entropy, np.float32).reshape(8, 8)[:h, :w]
        asked |= {(k, bx0 + cx, by0 + cy) for k, cx, cy in wk.asked}
        took |= wk.took
    return acs, ent, asked, took


def valid_tiling(acs):
    """Every block belongs to exactly one transform whose first block carries the bit, all of it inside the frame and inside
    one 64x64 tile."""
    acs = np.asarray(acs)
    yb, xb = acs.shape
    covered_of = {num: (cx, cy) for _, num, cx, cy in KINDS}
    owner = np.zeros((yb, xb), np.int32)
    for y in range(yb):
        for x in range(xb):
            if not acs[y, x] & 1:
                continue
            if int(acs[y, x]) >> 1 not in covered_of:
                return False
            cx, cy = covered_of[int(acs[y, x]) >> 1]
            if x + cx > xb or y + cy > yb or x % 8 + cx > 8 or y % 8 + cy > 8:
                return False
            if not np.all(acs[y:y + cy, x:x + cx] >> 1 == acs[y, x] >> 1):
                return False
            if np.count_nonzero(acs[y:y + cy, x:x + cx] & 1) != 1:
                return False
            owner[y:y + cy, x:x + cx] += 1
    return bool(np.all(owner == 1))
