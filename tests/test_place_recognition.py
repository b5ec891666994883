"""Loop retrieval by appearance (loopy_slam_amd/place.py and LoopCloser.appearance_candidates) on frames of the 'textured' synthetic room,
against the NumPy referee tests/place_referee.py: 240 x 320 frames on synthetic.loop_pose(k, 200).

The scores are ratios of integers, so the device's equal the referee's exactly and the expected candidate lists are the rule of
loop_closure.py applied to the referee's scores.  The default loop_closure.min_score is MEASURED: midway between the highest referee score of
two views 50 or more poses apart and the lowest of two views within 5 poses (figures: profiles/place_recognition.md)."""
import copy

import numpy as np
import pytest
import torch

import place_referee as R
import util
from loopy_slam_amd import config, slam, synthetic
from loopy_slam_amd import loop_closure as LC

torch.set_num_threads(1)
INTR = dict(H=240, W=320, fx=258.65, fy=258.25, cx=159.3, cy=127.65)        # synthetic.TUM_INTR at half size
SEGMENT_POSES = tuple(range(0, 200, 20))                                    # segments 0 .. 9
REVISIT, ELSEWHERE = 200.5, 150
NEAR_EXTRA = (5, 22, 102, 105)                                              # with 0, 20, 100 and 200.5: the pairs within 5 poses
MAX_HAMMING = LC.DEFAULTS['max_hamming']
_FRAMES, _REF = {}, {}


def frame(k):
    if k not in _FRAMES:
        _, color, c2w = synthetic.render_frame(k, intr=INTR, holes=0.0, scene='textured')
        _FRAMES[k] = (color, c2w)
    return _FRAMES[k]


def ref_desc(k):
    if k not in _REF:
        _REF[k] = R.describe(frame(k)[0].numpy())[1]
    return _REF[k]


def ref_score(a, b):
    return R.score(ref_desc(a), ref_desc(b), MAX_HAMMING)


def pose_gap(a, b):
    d = abs(a - b) % 200
    return min(d, 200 - d)


def separation():
    """(highest score of two views 50 or more poses apart, lowest of two within 5) over all pairs of the frames of this module."""
    if 'sep' not in _REF:
        ks = SEGMENT_POSES + (ELSEWHERE, REVISIT) + NEAR_EXTRA
        far = [ref_score(a, b) for i, a in enumerate(ks) for b in ks[i + 1:] if pose_gap(a, b) >= 50]
        near = [ref_score(a, b) for i, a in enumerate(ks) for b in ks[i + 1:] if pose_gap(a, b) <= 5]
        assert len(far) >= 30 and len(near) >= 6
        _REF['sep'] = (max(far), min(near))
    return _REF['sep']


_DEV = {}


def backend_of(eng):
    return eng.device.type


class _Npc:
    """What LoopCloser needs of a NeuralPointCloud when only candidates are asked for."""

    def __init__(self, eng):
        self.eng, self.capacity, self.n = eng, 1, 0


def closer_with(eng, poses, displaced_last=None, preload=False, **over):
    """A LoopCloser in the 'appearance' mode and the segment records of the frames `poses` (est_c2w = the true pose; the last one moved by
    `displaced_last` metres along x)."""
    lc = {'enabled': True, 'candidates': 'appearance'}
    lc.update({k: v for k, v in over.items() if k in LC.DEFAULTS})
    tr = {'min_dist': 1, 'kval': 2, 'dbow_filter': True, 'mult_dbow': 1.0}
    tr.update({k: v for k, v in over.items() if k in tr})
    closer = LC.LoopCloser({'loop_closure': lc, 'tracking': tr}, _Npc(eng))
    if preload:         # the descriptors of these frames as the first closer of this backend made them (describe_segments' bookkeeping)
        for k in poses:
            if (backend_of(eng), k) not in _DEV:
                _DEV[(backend_of(eng), k)] = closer.place.describe(frame(k)[0])[1]
            closer.place.add(_DEV[(backend_of(eng), k)])
            closer.seg_desc.append(_DEV[(backend_of(eng), k)])
            closer.self_score.append(-1.0)
    segments = []
    for i, k in enumerate(poses):
        color, c2w = frame(k)
        est = c2w.clone()
        if displaced_last is not None and i == len(poses) - 1:
            est[0, 3] += displaced_last
        segments.append({'idx': 10 * i, 'color': color.to(eng.device), 'est_c2w': est.to(eng.device), 'gt_c2w': c2w.to(eng.device)})
    return closer, segments


def expected(poses, self_score, min_dist=1, kval=2, dbow_filter=True, mult_dbow=1.0, min_score=LC.DEFAULTS['min_score']):
    """The rule on the referee's scores."""
    s = len(poses) - 1
    sc = [ref_score(poses[s], poses[t]) for t in range(s)]
    ok = [t for t in range(s) if abs(s - t) > min_dist and sc[t] > min_score and (not dbow_filter or sc[t] > mult_dbow * self_score[t])]
    ok.sort(key=lambda t: (-sc[t], t))
    return [(s, t) for t in ok[:kval]], sc


# ------------------------------------------------------------------------------------------------ the scene carries the feature
def test_textured_scene():
    intr = dict(H=60, W=80, fx=64.0, fy=64.0, cx=39.5, cy=29.5)
    dt, ct, pt = synthetic.render_frame(3, intr=intr, holes=0.0, scene='textured')
    df, cf, pf = synthetic.render_frame(3, intr=intr, holes=0.0, scene='furnished')
    assert torch.equal(dt, df) and torch.equal(pt, pf)                      # the furnished geometry
    ratio = ct / cf.clamp(min=1e-6)
    assert float(ct.min()) >= 0.0 and float((ct - cf).max()) <= 1e-6 and float(ratio[cf > 0.05].min()) >= 0.25 - 1e-4
    assert len(torch.unique((ratio[cf > 0.05] * 1000).round())) > 50        # many brightness cells
    # FAST-9 corners at 240 x 320, level 0: the scene is what the descriptor needs
    n = int(R.corners(R.grey_image(frame(0)[0].numpy()))[0].sum())
    print(f'textured frame 0 at 240 x 320: {n} FAST-9 corners at threshold 20')
    assert n >= 500


def test_min_score_default_is_measured():
    far, near = separation()
    print(f'referee scores: highest of two views >= 50 poses apart {far:.3f}, lowest of two views within 5 poses {near:.3f}; '
          f'default min_score {LC.DEFAULTS["min_score"]}')
    assert near - far >= 0.1
    assert abs(LC.DEFAULTS['min_score'] - 0.5 * (far + near)) <= 0.0051


# ------------------------------------------------------------------------------------------------ retrieval
@pytest.mark.parametrize('backend', util.backends())
def test_appearance_finds_the_loop_the_poses_miss(backend):
    eng = util.make_engine(backend)
    poses = SEGMENT_POSES + (REVISIT,)
    closer, segments = closer_with(eng, poses, displaced_last=3.0)
    assert closer.pose_candidates(segments) == []                           # the drifted pose hides the loop
    pairs = closer.appearance_candidates(segments)
    want, sc = expected(poses, [-1.0] * 11)
    print('scores of segment 10 against 0 .. 9:', np.round(closer.last_scores[:10], 3).tolist(), '->', pairs)
    assert pairs and pairs[0] == (10, 0)
    assert pairs == want
    assert np.array_equal(closer.last_scores[:10], np.array(sc))            # ratios of equal integers
    assert closer.last_scores[10] == 1.0                                    # a keyframe against itself
    assert len(closer.seg_desc) == 11 and closer.place.n_segments == 11
    kp, desc = closer.place.describe(segments[0]['color'])
    assert np.array_equal(desc.cpu().numpy().view(np.uint32), ref_desc(0)) and kp.shape == (len(ref_desc(0)), 4)


@pytest.mark.parametrize('backend', util.backends())
def test_no_false_loop(backend):
    eng = util.make_engine(backend)
    poses = SEGMENT_POSES[:6] + (ELSEWHERE,)
    closer, segments = closer_with(eng, poses)
    assert closer.appearance_candidates(segments) == []
    assert closer.last_scores[:6].max() < LC.DEFAULTS['min_score']
    assert expected(poses, [-1.0] * 7)[0] == []


@pytest.mark.parametrize('backend', util.backends())
def test_filters(backend):
    eng = util.make_engine(backend)
    poses = SEGMENT_POSES + (REVISIT,)
    none = [-1.0] * 11
    loose = dict(min_score=0.0)                    # every segment with a match at all passes
    cases = [
        (dict(), none), (dict(min_dist=9), none), (dict(min_dist=10), none),
        (dict(kval=1, **loose), none), (dict(kval=3, **loose), none), (dict(kval=20, **loose), none), (dict(kval=20, min_dist=3, **loose), none),
    ]
    high = list(none)
    high[0] = 0.9                                  # segment 0's own frames score higher among themselves than the revisit does
    low = [0.01] * 11
    cases += [(dict(), high), (dict(dbow_filter=False), high), (dict(mult_dbow=0.5), high), (dict(kval=20, **loose), high),
              (dict(kval=20, mult_dbow=20.0, **loose), low), (dict(kval=20, mult_dbow=20.0, **loose), none)]
    lists = []
    for over, self_score in cases:
        closer, segments = closer_with(eng, poses, preload=True, **over)
        closer.self_score = list(self_score)
        got = closer.appearance_candidates(segments)
        want, _ = expected(poses, self_score, **over)
        print(over, [s for s in self_score if s >= 0], '->', got)
        assert got == want
        lists.append(got)
    # the cases do differ as the rule says
    assert lists[0][0] == (10, 0) and lists[1][0] == (10, 0) and (10, 0) not in lists[2] and lists[2] == []
    assert len(lists[3]) == 1 and len(lists[4]) == 3 and len(lists[5]) > 3 and all(t <= 8 for _, t in lists[5])
    assert all(t <= 6 for _, t in lists[6]) and len(lists[6]) < len(lists[5])
    assert (10, 0) not in lists[7] and lists[8][0] == (10, 0) and lists[9][0] == (10, 0)
    assert (10, 0) not in lists[10] and len(lists[10]) == len(lists[5]) - 1
    assert lists[11] == [(10, 0)]                  # a threshold of 20 x 0.01 = 0.2: the revisit alone is above it
    assert lists[12] == lists[5]                   # self_score = -1 (no frames yet) lets every score pass


@pytest.mark.parametrize('backend', util.backends())
def test_self_score_is_a_running_minimum(backend):
    eng = util.make_engine(backend)
    closer, segments = closer_with(eng, (0,))
    closer.describe_segments(segments)
    assert closer.self_score == [-1.0]
    seen = []
    for k in (5, REVISIT, 22):
        closer.on_mapped_frame(frame(k)[0].to(eng.device), segments)
        seen.append(ref_score(k, 0))
        assert closer.self_score == [min(seen)]
    assert closer.place.n_segments == 1                                       # mapped frames do not join the database


# ------------------------------------------------------------------------------------------------ through slam.Mapper
def mapper_cfg(candidates, n_frames=6, segment_size=2):
    """The small budget of tests/test_loop_closure.py::small_cfg on a 120 x 160 camera looking at the textured room."""
    cfg = copy.deepcopy(config.load_config('configs/Synthetic/room.yaml', 'configs/point_slam.yaml'))
    cfg['cam'].update(H=120, W=160, fx=130.0, fy=130.0, cx=79.5, cy=59.5)
    cfg['tracking'].update(ignore_edge_W=2, ignore_edge_H=2, pixels=48, iters=3, min_dist=1, mult_dbow=0.1)
    cfg['mapping'].update(pixels=64, pixels_adding=400, iters=3, iters_first=6, geo_iter_first=2, every_frame=2, keyframe_every=2,
                          mapping_window_size=4, segment_strategy='fixed', color_refine=False)
    cfg['pointcloud'].update(radius_add=0.12, radius_query=0.24, radius_min=0.06)
    cfg['data'].update(n_frames=n_frames, scene='textured')
    cfg['mapping']['fixed_segment_size'] = segment_size
    cfg['loop_closure'] = {'enabled': True, 'candidates': candidates, 'min_score': 0.02}
    return cfg


def run_state(ps):
    npc = ps.npc
    return (npc._pos[:npc.n].clone(), npc._geo[:npc.n].clone(), npc._col[:npc.n].clone(), npc._seg[:npc.n].clone(),
            ps.estimate_c2w_list.clone(), torch.stack([s['est_c2w'].cpu() for s in ps.mapper.segments]))


@pytest.mark.parametrize('backend', util.backends())
def test_through_the_mapper(backend):
    eng = util.make_engine(backend)
    # 'pose': no recogniser, and the run is the one the pose rule gives as a caller's function (the path a callable always took)
    ps = slam.Point_SLAM(mapper_cfg('pose'), None, eng=eng)
    ps.run()
    assert ps.mapper.closer.place is None and ps.mapper.closer.seg_desc == []
    holder = {}
    ps2 = slam.Point_SLAM(mapper_cfg(lambda segments: holder['closer'].pose_candidates(segments)), None, eng=eng)
    holder['closer'] = ps2.mapper.closer
    ps2.run()
    assert ps2.mapper.closer.place is None
    for a, b in zip(run_state(ps), run_state(ps2)):
        assert torch.equal(a, b)
    # 'appearance'
    ps3 = slam.Point_SLAM(mapper_cfg('appearance', n_frames=10, segment_size=4), None, eng=eng)
    closer = ps3.mapper.closer
    log, inner = [], closer.appearance_candidates

    def logged(segments):
        pairs = inner(segments)
        log.append((pairs, closer.last_scores.copy(), list(closer.self_score)))
        return pairs
    closer.appearance_candidates = logged
    ps3.run()
    segments = ps3.mapper.segments
    assert [s['idx'] for s in segments] == [0, 4, 8]
    assert closer.place is not None and closer.place.n_segments == 3 and len(closer.seg_desc) == 3
    assert all(int(d.shape[0]) > 0 for d in closer.seg_desc)
    assert all(s >= 0 for s in closer.self_score)                              # frames 2, 6 and 9 are second mapped frames of their segments
    assert len(log) == 1                                                       # the closure of segment 2 (fewer than 3 segments: none)
    for pairs, scores, self_score in log:
        print('proposed', pairs, 'scores', np.round(scores, 3).tolist(), 'self', np.round(self_score, 3).tolist())
        assert len(pairs) <= closer.kval
        for s, t in pairs:
            assert s == len(scores) - 1 and abs(s - t) > 1 and scores[t] > 0.02 and scores[t] > 0.1 * self_score[t]
