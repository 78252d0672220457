"""Host model of k_tower3's B-fragment LDS reads (csrc/gmz_net.hip Img3 / tile_pos / lastpos) per board size.

For every position tile, tap and k-step it forms the 64 lane addresses of the ds_read_b128 and counts, per
hardware lane group (four non-contiguous groups of 16 lanes), the worst number of distinct addresses that
share one 16-byte slot of the 256-byte bank row: 1 = conflict-free.  15x15 runs the border-tile order
(remap15), which gmz_common.h models on its own; it is skipped here.

    python tools/tower_bank_model.py            # sizes 5..19 with the library's boards-per-workgroup
"""
NB = {5: 5, 6: 2, 7: 2, 8: 2, 9: 2, 10: 2}  # TowerCfg<H>::NB (1 elsewhere)
GROUPS = [list(range(0, 4)) + list(range(12, 16)) + list(range(20, 28)),
          list(range(4, 12)) + list(range(16, 20)) + list(range(28, 32))]
GROUPS += [[l + 32 for l in g] for g in GROUPS]
PS = 272


def sigma16(j):
    return j ^ 4 if j < 8 else j


def model(H, nb):
    A, HP = H * H, H + 2
    RS = HP * PS - 32
    img = ((HP - 1) * RS + HP * PS + 255) // 256 * 256
    one = 2 * img + 2 * 128 * 4 + 9 * 128 * 4 > 163840
    BB = (1 if one else 2) * img
    bbase = lambda b: b * BB + (((b * A) & 15) * 16 if nb > 1 else 0)  # noqa: E731
    tiles = (nb * A + 15) // 16
    lastpos = bbase(nb - 1) + ((A - 1) // H) * RS + ((A - 1) % H) * PS
    worst, where = 1, None
    for pt in range(tiles):
        for tap in range(9):
            for ks in range(4):
                addr = []
                for lane in range(64):
                    gp = pt * 16 + sigma16(lane & 15)
                    b, p = divmod(gp, A)
                    base = bbase(b) + (p // H) * RS + (p % H) * PS if b < nb else lastpos
                    cg = (0, 8, 1, 9)[lane >> 4]
                    addr.append(base + cg * 16 + (tap // 3) * RS + (tap % 3) * PS + ks * 32)
                for g in GROUPS:
                    slots = {}
                    for l in g:
                        slots.setdefault((addr[l] // 16) % 16, set()).add(addr[l])
                    w = max(len(s) for s in slots.values())
                    if w > worst:
                        worst, where = w, (pt, tap, ks)
    return tiles, worst, where


if __name__ == "__main__":
    for H in range(5, 20):
        if H == 15:
            print("15x15: border-tile order (remap15), modelled in gmz_common.h")
            continue
        nb = NB.get(H, 1)
        tiles, worst, where = model(H, nb)
        print("%2dx%-2d NB %d: %2d tiles, worst %d-way%s" % (H, H, nb, tiles, worst,
                                                           "" if worst == 1 else " at (tile, tap, k-step) %s" % (where,)))
