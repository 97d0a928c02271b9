"""Plain-loop restatement of the pose verification (the header of sam6d_amd/csrc/s6d_verify.hip), independent of
sam6d_amd/pem/verify.py: Python loops over instances and pixels, np.float32 arithmetic for z and d, Python integers for the words,
Python floats (doubles) for the comparisons of the selection."""
import numpy as np

NAMES = ("rendered", "missing", "inlier", "occluded", "behind", "det", "det_rendered", "det_inlier")


def evidence(render, depth_obs, obs_index, depth_unit, tau, masks=None):
    """-> dict(counts (N,8) int64, inlier (N,words) uint64, span (N,2) int64, cls (N,H,W) int8: -1 not rendered, 0 missing, 1 inlier,
    2 occluded, 3 behind)."""
    render = np.asarray(render, np.float32)
    depth_obs = np.asarray(depth_obs, np.float32)
    N, H, W = render.shape
    plane = H * W
    words = (plane + 63) // 64
    unit, tau = np.float32(depth_unit), np.float32(tau)
    counts = np.zeros((N, 8), np.int64)
    inlier = [[0] * words for _ in range(N)]
    cls = np.full((N, H, W), -1, np.int8)
    with np.errstate(all="ignore"):
        for n in range(N):
            r_, z_ = render[n].reshape(-1), depth_obs[int(obs_index[n])].reshape(-1)
            m_ = None if masks is None else np.asarray(masks[n]).reshape(-1)
            for p in range(plane):
                r = r_[p]
                rendered = bool(r > 0)
                z = np.float32(z_[p] * unit)
                measured = bool(z > 0) and bool(z < np.float32(np.inf))
                det = m_ is not None and m_[p] != 0
                c = -1
                if rendered:
                    if not measured:
                        c = 0
                    else:
                        d = np.float32(z - r)
                        c = 1 if abs(d) <= tau else (2 if d < -tau else 3)
                        assert c != 3 or d > tau
                    counts[n, 0] += 1
                    counts[n, 1 + c] += 1
                    if c == 1:
                        inlier[n][p >> 6] |= 1 << (p & 63)
                cls[n, p // W, p % W] = c
                if det:
                    counts[n, 5] += 1
                    counts[n, 6] += rendered
                    counts[n, 7] += c == 1
    span = np.zeros((N, 2), np.int64)
    for n in range(N):
        nz = [j for j in range(words) if inlier[n][j]]
        span[n] = (nz[0], nz[-1]) if nz else (words, -1)
    return dict(counts=counts, inlier=np.array(inlier, np.uint64).reshape(N, words), span=span, cls=cls)


def scores(counts, with_masks):
    """-> (score, fit, sil) float64 (N,)."""
    N = len(counts)
    fit, sil = np.ones(N), np.ones(N)
    for n in range(N):
        c = [int(x) for x in counts[n]]
        fit[n] = float(c[2]) / float(max(c[2] + c[4], 1))
        if with_masks:
            sil[n] = float(c[6]) / float(max(c[5] + c[0] - c[6], 1))
    return fit * sil, fit, sil


def default_order(score, counts, frame, n_frames):
    """-> (order, frame_start): frame by frame, descending score, then descending inlier count, then ascending index."""
    order, start = [], [0]
    for b in range(n_frames):
        order += sorted([n for n in range(len(score)) if frame[n] == b], key=lambda n: (-float(score[n]), -int(counts[n][2]), n))
        start.append(len(order))
    return np.array(order, np.int32), np.array(start, np.int64)


def key_order(key, frame, n_frames):
    order, start = [], [0]
    for b in range(n_frames):
        order += sorted([n for n in range(len(key)) if frame[n] == b], key=lambda n: (-float(key[n]), n))
        start.append(len(order))
    return np.array(order, np.int32), np.array(start, np.int64)


def select(inlier, counts, order, frame_start, flagged, min_inliers, min_fit, min_fresh):
    """-> (status (N,), fresh (N,)) int64."""
    N, words = inlier.shape
    mf, mr = float(np.float32(min_fit)), float(np.float32(min_fresh))
    status, fresh = np.full(N, 4, np.int64), np.zeros(N, np.int64)
    for b in range(len(frame_start) - 1):
        claimed = [0] * words
        for k in range(int(frame_start[b]), int(frame_start[b + 1])):
            n = int(order[k])
            w = [int(x) for x in inlier[n]]
            fr = sum(bin(w[j] & ~claimed[j]).count("1") for j in range(words))
            rendered, inl, beh = int(counts[n][0]), int(counts[n][2]), int(counts[n][4])
            if rendered == 0 or (flagged is not None and flagged[n]):
                st = 4
            elif inl < int(min_inliers):
                st = 1
            elif float(inl) < mf * float(inl + beh):
                st = 2
            elif float(fr) < mr * float(inl):
                st = 3
            else:
                st = 0
                claimed = [claimed[j] | w[j] for j in range(words)]
            status[n], fresh[n] = st, fr
    return status, fresh


def verify(render, depth_obs, frame, depth_unit, tau, masks, flagged, min_inliers, min_fit, min_fresh, order_by=None):
    """The whole step from the renders -> dict(status, fresh, score, fit, sil, counts, order, frame_start, keep)."""
    ev = evidence(render, depth_obs, frame, depth_unit, tau, masks)
    score, fit, sil = scores(ev["counts"], masks is not None)
    M = len(depth_obs)
    order, start = default_order(score, ev["counts"], frame, M) if order_by is None else key_order(order_by, frame, M)
    status, fresh = select(ev["inlier"], ev["counts"], order, start, flagged, min_inliers, min_fit, min_fresh)
    return dict(status=status, fresh=fresh, score=score, fit=fit, sil=sil, counts=ev["counts"], order=order, frame_start=start,
                keep=status == 0, inlier=ev["inlier"], span=ev["span"])
