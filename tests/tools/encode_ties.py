"""VQ codebooks whose entries tie, for the encoder's tie rules (tests/tools/make_golden_encode_ties.py, tests/test_gpu_encode_ties.py).

The searches of the encoder decide equal distances by the lower index, as the reference's strict `<` over ascending entries does.  On the device an
entry's index is 256 kk + 4 lane + e (encode_kernels.hip.h: enc_search5): a lane compares its sixteen entries in ascending (kk, e), and the
wavefront's butterfly (enc_wave_argmin) compares lanes at the distances 32, 16, 8, 4, 2, 1.  So the stage codebooks hold each of 256 vectors at
four positions -- a GROUP --, and the groups are placed so that the pairs inside them are of every kind a tie can take on the device:

  same_lane   same kk and lane, another e
  kk          another kk (idx and idx + 256 k)
  xor32 .. xor1   same kk, lanes l and l ^ D: the two sides of the butterfly step of distance D
  neighbour   same kk, lanes l and l + 1 (half of them are xor1 pairs as well)

A group is the coset {a, a ^ m0, a ^ m1, a ^ m0 ^ m1} of the two masks of one TYPE around a seeded index a: of the types whose coset is still free
the one with the fewest groups so far; where none is, any three free indices.  place_groups' census is asserted in make().  ceps_codebook_diff4 (entry i is searched against target variant i & 3, all positive signs before all negative ones):

  quarter 1 = quarter 0      the same variant, a tie across quarters: the copy never wins
  quarter 2 = -quarter 0     the positive pass of i + 2048 ties the negative pass of i (and the other way round): no negative sign in quarters 0..2
  quarter 3                  entries 8 j + 4 and 8 j + 5 (variants 0 and 1, whose targets are the same vector) are equal; ZERO_ROWS are
                             zero, which tie with themselves across the sign
"""
import numpy as np

SEED = 77
NB1, NB = 17, 18
# two generators of each type's mask set, as (kk, lane, e) bit positions of the index: e = bits 0..1, lane = bits 2..7, kk = bits 8..9
TYPES = {
    "e": (1, 2),                      # same lane, e = 0..3
    "kk": (256, 512),                 # kk = 0..3
    "lane32_16": (32 << 2, 16 << 2),
    "lane8_4": (8 << 2, 4 << 2),
    "lane2_1": (2 << 2, 1 << 2),
    "kk_lane32": (256, 32 << 2),      # two kk x the two sides of the first butterfly step
    "e_lane1": (1, 1 << 2),           # two e x two neighbouring lanes
}
KINDS = ("same_lane", "kk", "xor32", "xor16", "xor8", "xor4", "xor2", "xor1", "neighbour")
ZERO_ROWS = (3072 + 4 * 10 + 2, 3072 + 4 * 77 + 3, 3072 + 4 * 140 + 2, 3072 + 4 * 201 + 3)


def pair_kinds(a, b):
    """the kinds of the pair of stage-codebook indices (a, b), a != b"""
    ka, la, kb, lb = a >> 8, (a >> 2) & 63, b >> 8, (b >> 2) & 63
    out = []
    if ka != kb:
        out.append("kk")
        return out
    if la == lb:
        out.append("same_lane")
        return out
    if (la ^ lb) in (32, 16, 8, 4, 2, 1):
        out.append("xor%d" % (la ^ lb))
    if abs(la - lb) == 1:
        out.append("neighbour")
    return out


def place_groups(rng):
    """-> group [1024] (0..255) of every index, and the type name of every group"""
    names = list(TYPES)
    group = np.full(1024, -1, np.int64)
    types = []
    free = list(rng.permutation(1024))
    g = 0
    while g < 256:
        a = int(free.pop())
        if group[a] >= 0:
            continue
        for name in sorted(names, key=lambda t: (types.count(t), names.index(t))):      # the type with the fewest groups so far whose coset around a is free
            m0, m1 = TYPES[name]
            members = [a, a ^ m0, a ^ m1, a ^ m0 ^ m1]
            if all(group[m] < 0 for m in members):
                break
        else:                                   # none is: any three free indices
            rest = [int(x) for x in np.flatnonzero(group < 0) if x != a][:3]
            members, name = [a] + rest, "any"
        group[members] = g
        types.append(name)
        g += 1
    assert (group >= 0).all() and np.bincount(group, minlength=256).tolist() == [4] * 256
    return group, types


def placement_census(group):
    """pairs inside the groups, by kind"""
    out = dict.fromkeys(KINDS, 0)
    for g in range(256):
        m = np.flatnonzero(group == g).tolist()
        for i in range(4):
            for j in range(i + 1, 4):
                for k in pair_kinds(m[i], m[j]):
                    out[k] += 1
    return out


def make(seed=SEED):
    """-> dict(cbs = (cb1, cb2, cb3, cbd) float32, groups = [3][1024] the group of every stage-codebook index, types = [3][256] names)"""
    rng = np.random.default_rng([seed, 0x71E5])
    cbs, groups, types = [], [], []
    for scale in (1.2, 0.5, 0.25):
        group, tnames = place_groups(rng)
        census = placement_census(group)
        assert all(census[k] >= 40 for k in KINDS), census         # every kind of pair is there to be hit
        assert all(tnames.count(t) >= 16 for t in TYPES), tnames
        base = (rng.standard_normal((256, NB1)) * scale).astype(np.float32)
        cbs.append(np.ascontiguousarray(base[group]))
        groups.append(group)
        types.append(tnames)
    q0 = (rng.standard_normal((1024, NB)) * 0.3).astype(np.float32)
    q3 = (rng.standard_normal((1024, NB)) * 0.3).astype(np.float32)
    q3[4::8] = q3[5::8]                                              # rows 8 j + 4 and 8 j + 5: variant 0 = variant 1
    for z in ZERO_ROWS:
        q3[z - 3072] = 0.0
    cbd = np.ascontiguousarray(np.concatenate([q0, q0, -q0, q3]))
    assert np.array_equal(cbd[1024:2048], cbd[:1024]) and np.array_equal(cbd[2048:3072], -cbd[:1024])
    assert all(np.array_equal(cbd[3072 + 8 * j + 4], cbd[3072 + 8 * j + 5]) for j in range(128))
    return dict(cbs=(cbs[0], cbs[1], cbs[2], cbd), groups=np.stack(groups), types=types)


def census(packets, ties):
    """what the packets of an encoder run under these codebooks show of the tie rules (make_golden_encode_ties.py asserts it of the reference)"""
    import make_golden_encode as mge
    f = mge.packet_fields(packets)
    out = dict(packets=int(f["e0"].size))
    kinds = dict.fromkeys(KINDS, 0)
    for s, name in enumerate(("e0", "e1", "e2")):
        group = ties["groups"][s]
        members = np.stack([np.flatnonzero(group == g) for g in range(256)])        # ascending
        won = f[name].reshape(-1)
        out[name + "_lowest"] = int((members[group[won], 0] == won).sum())
        for w, n in zip(*np.unique(won, return_counts=True)):
            for t in members[group[w]].tolist():
                if t != w:
                    for k in pair_kinds(int(w), t):
                        kinds[k] += int(n)
    out["kinds"] = kinds
    mid = f["mid"].reshape(-1)
    idx, neg = mid & 4095, mid >= 4096
    out["mid_in_copied_quarter"] = int(((idx >> 10) == 1).sum())
    out["mid_negative_with_positive_twin"] = int((neg & (idx < 3072)).sum())
    out["mid_pos"], out["mid_neg"] = int((~neg).sum()), int(neg.sum())
    q3 = idx[idx >= 3072] - 3072
    out["mid_second_of_equal_pair"] = int((q3 % 8 == 5).sum())      # 8 j + 5 equals 8 j + 4, which comes first
    out["mid_first_of_equal_pair"] = int((q3 % 8 == 4).sum())
    out["mid_zero_row"] = int(np.isin(idx, ZERO_ROWS).sum())
    out["mid_zero_row_negative"] = int((np.isin(idx, ZERO_ROWS) & neg).sum())
    out["corr_ids"] = sorted(set(f["corr"].reshape(-1).tolist()))
    out["interp_ids"] = sorted(set(f["interp"].reshape(-1).tolist()))
    out["pitch_min"], out["pitch_max"] = int(f["pitch"].min()), int(f["pitch"].max())
    out["c0_max"] = int(f["c0"].max())
    return out


def interp_census(packets, feats, cbs):
    """double_interp_search (src/lpcnet_enc.c:379-400) recomputed in float32 from one stream's packets [P][8] and its unquantised cepstra (feats
    [4P][>=18]: lpcnet_compute_features of the same PCM; frames 0 and 2 enter the search as they are) -> (interp ids as the search picks them, the
    number of packets in which the forbidden id 7 had the strictly smallest distance and was passed over)"""
    import make_golden_encode as mge
    f = mge.packet_fields(packets)
    cb1, cb2, cb3, cbd = cbs
    P, one = packets.shape[0], np.float32(1)
    q3 = np.zeros((P + 1, NB), np.float32)                          # vq_mem entering packet p; slot p + 1: the quantised frame 3
    q3[1:, 0] = (f["c0"] - 64).astype(np.float32) / np.float32(4)
    q3[1:, 1:] = (cb1[f["e0"]] + cb2[f["e1"]]) + cb3[f["e2"]]
    left, right = q3[:-1], q3[1:]
    idx, neg = f["mid"] & 4095, f["mid"] >= 4096
    v = idx & 3
    half = np.float32(.5)
    pred = np.where((v < 2)[:, None], half * (left + right), np.where((v == 2)[:, None], left, right))
    q1 = pred + np.where(neg, -one, one)[:, None] * cbd[idx]
    x0, x2 = feats[0::4, :NB], feats[2::4, :NB]

    def dist(x, p):
        e, d = x - p, np.zeros(P, np.float32)
        for k in range(NB):
            d = d + e[:, k] * e[:, k]
        return d
    d0 = [dist(x0, half * (left + q1)), dist(x0, left), dist(x0, q1)]
    d1 = [dist(x2, half * (q1 + right)), dist(x2, q1), dist(x2, right)]
    best, mind = np.zeros(P, np.int64), np.full(P, 1e15, np.float32)
    for i in range(3):
        for j in range(3):
            if 3 * i + j != 7:
                d = d0[i] + d1[j]
                take = d < mind
                best, mind = np.where(take, 3 * i + j, best), np.where(take, d, mind)
    return best - (best >= 7), int(((d0[2] + d1[1]) < mind).sum())


def conditions(c):
    """the conditions of the fixture -> list of the ones that fail (empty: all hold)"""
    bad = []
    for name in ("e0", "e1", "e2"):
        if c[name + "_lowest"] != c["packets"]:
            bad.append("%s: %d of %d winners are the lowest index of their group" % (name, c[name + "_lowest"], c["packets"]))
    bad += ["pair kind %s separates the winner from a twin %d times (< 10)" % (k, v) for k, v in c["kinds"].items() if v < 10]
    if c["mid_in_copied_quarter"]:
        bad.append("vq_mid in the copied quarter")
    if c["mid_negative_with_positive_twin"]:
        bad.append("a negative-sign vq_mid whose positive twin exists")
    if c["mid_second_of_equal_pair"] or c["mid_zero_row_negative"]:
        bad.append("the later of two equal entries of quarter 3 won")
    if not (c["mid_pos"] and c["mid_neg"]):
        bad.append("one sign of vq_mid does not occur")
    if c["corr_ids"] != [0, 1, 2, 3]:
        bad.append("corr ids %s" % c["corr_ids"])
    if not (c["pitch_min"] == 0 and c["pitch_max"] == 63 and c["c0_max"] == 127):
        bad.append("clamps: pitch %d .. %d, c0 up to %d" % (c["pitch_min"], c["pitch_max"], c["c0_max"]))
    return bad
