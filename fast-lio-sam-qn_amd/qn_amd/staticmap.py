"""The static map - the corrected map without the records other keyframes saw through: the numpy twin of csrc/qn_staticmap.hip (qn_kf_static_classify /
qn_kf_static_points / qn_kf_build_map_static) and its specification.  Pure numpy, no GPU, built on freespace.py (tables, transform, classify, range_images)
and scancontext.relative_pose.

Whatever moved while the sensor drove past stays in the corrected map as a ghost trail.  A record of keyframe i is transient if, carried with the corrected
poses into a neighbouring keyframe j's sensor frame, it lies where j's rays passed on their way to a farther surface: class 2, SEEN THROUGH, of the free-space
check, by the same projection, the same images and the same tolerances as the loop check.

  list         ids[0 .. count) with poses[0 .. count), each 4x4 f64, sensor -> world: the list build_map takes.  Ids may repeat.  A list position is an ENTRY.
  witnesses    of entry e: wit[wit_off[e] .. wit_off[e + 1]), entry positions (CSR).  The caller may pass any list; a witness never has the entry's own keyframe
               id; at most MAX_WITNESSES = 255 per entry.  witnesses() makes the default list: the nearest entries of another keyframe.
  votes        of record p of entry e, over its witnesses w in list order: M = scancontext.relative_pose(P_w, P_e), the point freespace.transform(p, M) in f64
               and unrounded, its class by freespace.classify against the images of keyframe ids[w] under the range parameters.  seen_through[p] = the number of
               witnesses giving class 2, agree[p] = the number giving class 4, both uint8 (exact under the cap).
  rule         StaticParams (qn_static_params): min_see_through (>= 1, default 2), agree_weight (default 1).  Record p is REMOVED iff
               seen_through >= min_see_through and seen_through > agree_weight * agree - integers only.  A record with a non-finite coordinate is dropped by
               every witness (class 0), gets no vote and is never removed: the map pipeline treats it as it always did.
  static map   by definition build_map of the same list, poses and leaf over keyframes from which the removed records have been deleted (order and intensity
               kept; an entry with nothing left contributes nothing).  static_clouds() gives those keyframes."""
from dataclasses import dataclass
import numpy as np
from . import freespace, scancontext

MAX_WITNESSES = 255


@dataclass
class StaticParams:
    min_see_through: int = 2
    agree_weight: int = 1


def params_ok(rule):
    """the checks of qn_kf_static_classify on its rule"""
    return 1 <= int(rule.min_see_through) <= 0xFFFFFFFF and 0 <= int(rule.agree_weight) <= 0xFFFFFFFF


def _poses(poses, count):
    P = np.asarray(poses, np.float64).reshape(-1, 4, 4)
    if len(P) != count:
        raise ValueError("staticmap: %d entries but %d poses" % (count, len(P)))
    return P


def witnesses(ids, poses, radius, max_k):
    """-> (wit_off (count + 1,) uint32, wit uint32): for entry e the up to max_k other entries with a different id whose translation lies within `radius` of
    e's (squared f64 distance, summed x, y, z in order, <= radius * radius), ascending distance, ties to the lower position.  Host code, O(count^2)."""
    ids = [int(i) for i in np.asarray(ids).reshape(-1)]
    P = _poses(poses, len(ids))
    if not (0 <= int(max_k) <= MAX_WITNESSES):
        raise ValueError("staticmap.witnesses: max_k must be 0 .. %d" % MAX_WITNESSES)
    t = [[float(P[e, 0, 3]), float(P[e, 1, 3]), float(P[e, 2, 3])] for e in range(len(ids))]
    r2 = float(radius) * float(radius)
    off = [0]; wit = []
    for e in range(len(ids)):
        c = []
        for w in range(len(ids)):
            if ids[w] == ids[e]:
                continue
            dx, dy, dz = t[w][0] - t[e][0], t[w][1] - t[e][1], t[w][2] - t[e][2]
            d2 = (dx * dx + dy * dy) + dz * dz
            if d2 <= r2:
                c.append((d2, w))
        c.sort()
        wit += [w for _, w in c[:int(max_k)]]
        off.append(len(wit))
    return np.array(off, np.uint32), np.array(wit, np.uint32)


def window_witnesses(ids, W):
    """-> (wit_off, wit): the entries within W list positions of e (lower positions first) that carry another keyframe id - the neighbours in time"""
    ids = [int(i) for i in np.asarray(ids).reshape(-1)]
    off = [0]; wit = []
    for e in range(len(ids)):
        wit += [w for w in range(max(0, e - int(W)), min(len(ids), e + int(W) + 1)) if ids[w] != ids[e]]
        off.append(len(wit))
    return np.array(off, np.uint32), np.array(wit, np.uint32)


def check_witnesses(ids, wit_off, wit):
    """the checks of qn_kf_static_classify on its witness list -> (wit_off, wit) as uint32 arrays"""
    ids = np.asarray(ids).reshape(-1)
    off = np.asarray(wit_off, np.int64).reshape(-1); w = np.asarray(wit, np.int64).reshape(-1)
    if len(off) != len(ids) + 1 or (np.diff(off) < 0).any() or off[0] < 0 or off[-1] > len(w):
        raise ValueError("staticmap: wit_off must be count + 1 non-decreasing offsets into wit")
    if (np.diff(off) > MAX_WITNESSES).any():
        raise ValueError("staticmap: more than %d witnesses for an entry" % MAX_WITNESSES)
    for e in range(len(ids)):
        for x in w[off[e]:off[e + 1]]:
            if not (0 <= x < len(ids)) or ids[x] == ids[e]:
                raise ValueError("staticmap: witness %d of entry %d is no entry of another keyframe" % (x, e))
    return off.astype(np.uint32), w.astype(np.uint32)


def votes(clouds, images, ids, poses, wit_off, wit, p, tabs=None):
    """clouds[id] = the (n, >= 3) f32 records of keyframe id, images[id] = its (near, far) range images (needed for witnesses only)
    -> per entry (seen_through (n,) uint8, agree (n,) uint8)"""
    ids = [int(i) for i in np.asarray(ids).reshape(-1)]
    P = _poses(poses, len(ids))
    wit_off, wit = check_witnesses(ids, wit_off, wit)
    tabs = freespace.tables(p) if tabs is None else tabs
    out = []
    for e in range(len(ids)):
        cloud = np.asarray(clouds[ids[e]], np.float32)
        st = np.zeros(len(cloud), np.uint8); ag = np.zeros(len(cloud), np.uint8)
        for w in wit[wit_off[e]:wit_off[e + 1]]:
            if not len(cloud):
                break
            M = scancontext.relative_pose(P[w], P[e])
            near, far = images[ids[w]]
            cls, _ = freespace.classify(freespace.transform(cloud, M), near, far, p, tabs)
            st += cls == freespace.SEEN_THROUGH; ag += cls == freespace.AGREE
        out.append((st, ag))
    return out


def removed(seen_through, agree, rule=None):
    """the rule on the votes of one entry -> (n,) bool"""
    rule = StaticParams() if rule is None else rule
    if not params_ok(rule):
        raise ValueError("staticmap: bad rule %r" % (rule,))
    st = np.asarray(seen_through).astype(np.int64); ag = np.asarray(agree).astype(np.int64)
    return (st >= int(rule.min_see_through)) & (st > int(rule.agree_weight) * ag)


def classify(clouds, ids, poses, wit_off, wit, p, rule=None, images=None):
    """-> per entry dict(seen_through, agree, removed).  images: {id: (near, far)}; made here from the clouds for the witnesses' keyframes when None."""
    tabs = freespace.tables(p)
    idl = [int(i) for i in np.asarray(ids).reshape(-1)]
    if images is None:
        images = {}
        for w in np.asarray(wit, np.int64).reshape(-1):
            if 0 <= w < len(idl) and idl[w] not in images:
                images[idl[w]] = freespace.range_images(clouds[idl[w]], p, tabs)
    return [dict(seen_through=st, agree=ag, removed=removed(st, ag, rule)) for st, ag in votes(clouds, images, idl, poses, wit_off, wit, p, tabs)]


def static_clouds(clouds, ids, result):
    """-> per entry the records of its keyframe that were not removed, in order (all columns kept): the keyframes the static map is build_map of"""
    return [np.asarray(clouds[int(i)])[~r["removed"]] for i, r in zip(np.asarray(ids).reshape(-1), result)]
