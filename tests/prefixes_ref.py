"""Plain Python restatement of "which registered prefix does a prompt take" (include/gten_host_prefixes.h,
gten_host_prefixes_match; host/prefix_match.h) and the seeded cases tests/test_prefixes_cpu.py checks the library against."""
import random

OWN_MIN = 16          # ids a prompt must have behind a prefix to take the short way


def match(prefixes, prompt):
    """index of the longest of `prefixes` (lists; empty: not registered) that `prompt` begins with and has OWN_MIN ids behind; the
    lower index among equal lengths; -1: none"""
    best, best_len = -1, 0
    for i, p in enumerate(prefixes):
        if not p or len(p) + OWN_MIN > len(prompt):
            continue
        if list(prompt[:len(p)]) == list(p) and len(p) > best_len:
            best, best_len = i, len(p)
    return best


def cases(count=200, seed=20240917):
    """(prefixes, prompt) pairs: nested prefixes, equal-length prefixes (equal and different ids), prompts with 15 / 16 / 17 ids
    behind a prefix, an empty registry, holes in the registry, a prompt shorter than every prefix"""
    rng = random.Random(seed)
    ids = lambda n: [rng.randrange(0, 50) for _ in range(n)]           # (a small alphabet: accidental common beginnings happen)
    out = []
    while len(out) < count:
        kind = len(out) % 8
        n_pre = rng.randrange(1, 9)
        base = ids(rng.randrange(16, 60))
        pres = []
        for _ in range(n_pre):
            r = rng.random()
            if r < 0.2:
                pres.append([])                                        # a hole
            elif r < 0.5 and pres and pres[-1]:
                pres.append(pres[-1] + ids(rng.randrange(1, 40)))      # nested: begins with the previous one
            elif r < 0.65 and pres and pres[-1]:
                pres.append(list(pres[-1]))                            # equal length, equal ids
            elif r < 0.8 and pres and pres[-1]:
                p = list(pres[-1])
                p[-1] = (p[-1] + 1) % 50                               # equal length, other ids
                pres.append(p)
            else:
                pres.append(base[:rng.randrange(16, len(base) + 1)] if rng.random() < 0.5 else ids(rng.randrange(16, 60)))
        if kind == 0:
            pres = [[] for _ in pres] if rng.random() < 0.5 else []    # an empty registry
        live = [p for p in pres if p]
        if live and kind in (1, 2, 3):
            p = rng.choice(live)
            prompt = p + ids({1: 15, 2: 16, 3: 17}[kind])              # the 16-id rule at its edge
        elif live and kind == 4:
            prompt = max(live, key=len) + ids(rng.randrange(16, 40))   # behind the longest
        elif live and kind == 5:
            prompt = rng.choice(live)[:rng.randrange(1, 16)]           # shorter than a prefix
        elif live and kind == 6:
            p = list(rng.choice(live))
            p[rng.randrange(len(p))] = 50                              # differs inside the prefix
            prompt = p + ids(30)
        else:
            prompt = ids(rng.randrange(1, 120))
        rng.shuffle(pres)
        out.append((pres, prompt))
    return out
