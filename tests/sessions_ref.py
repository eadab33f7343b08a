"""The turn plan of DESIGN.md 3.17, restated independently of host/session_plan.h: which rows of a conversation the next turn
keeps and which it computes."""

WHOLE, CONTINUED, ONE_BY_ONE = 0, 1, 2
MIN_ROWS = 16


def plan(h, r, n_new, segmented=True):
    """history of h ids with r leading valid K / V rows, a turn of n_new ids: (rows kept, rows computed, path) or None"""
    total = h + n_new
    if min(h, r, n_new) < 0 or r > h or total < 1:
        return None
    ctx = min(r, total - 1)                  # the turn ends with a computed row: its logits pick the next id
    k = total - ctx
    if ctx == 0:
        return ctx, k, WHOLE
    # history + turn of at least 16 ids is a prompt the segmented path takes: the turn is a segment too (of fewer than 16
    # rows: filled up); a shorter conversation stays with the operators, as a prompt of fewer than 16 ids does
    return ctx, k, CONTINUED if (total >= MIN_ROWS and segmented) else ONE_BY_ONE


def cases(count=200, seed=20260117):
    """seeded (h, r, n_new, segmented) with the corners in front: no history, every row valid, an empty turn, 15 and 16 rows"""
    import random
    rnd = random.Random(seed)
    out = [(0, 0, 1, True), (0, 0, 16, True), (0, 0, 40, False),          # h = 0: the whole-prompt path
           (40, 40, 0, True), (40, 39, 0, True), (1, 1, 0, True),          # n_new = 0 (r = h: one row is computed again)
           (57, 57, 12, True), (300, 300, 16, True),                       # r = h
           (100, 99, 14, True), (100, 99, 15, True),                       # k = 15 and 16
           (100, 100, 15, True), (100, 100, 16, True), (100, 85, 0, True), (100, 84, 0, True),
           (100, 99, 15, False), (10, 10, 5, True), (10, 10, 6, True), (15, 14, 0, True), (16, 15, 0, True), (0, 0, 0, True), (5, 6, 1, True), (-1, 0, 3, True), (3, 0, -1, True)]
    while len(out) < count:
        h = rnd.choice([0, 1, 2, 15, 16, 17, rnd.randrange(0, 400)])
        r = rnd.choice([0, h, max(h - 1, 0), rnd.randrange(0, h + 1)])
        out.append((h, r, rnd.choice([0, 1, 14, 15, 16, 17, rnd.randrange(0, 120)]), rnd.random() < 0.8))
    return out[:count]
