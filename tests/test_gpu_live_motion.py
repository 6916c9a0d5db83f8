"""-m gpu: live.LiveGaze(motion=...) -- the tracker's constant-velocity model under the live chain, with the engine, frames and crop size of
tests/test_gpu_live.py (tests/live_gpu_common.py).  One camera x 4 slots; a person walks 6 pixels a tick and is not detected in ticks 6 and 7.
  the plain tracker   the slot coasts at x = 34; tick 8's box at x = 52 overlaps it with IoU 6 * 24 / (1152 - 144) = 1 / 7 < 0.3: a second id
  gain 1, decay 1     v = 6 after tick 1, every later box is predicted exactly: ONE id, and the crops of ticks 6 and 7 are cut where the
                      person is (x = 40, 46), not where they were last seen
Every comparison is bit for bit."""
import numpy as np
import pytest
import torch

from mcgaze_amd import live
from mcgaze_amd import pipeline as P
from tests import live_cases as LC
from tests import track_cases as TC
from tests.live_gpu_common import ALPHA, CAMS, dev, make_engine, make_pipe, same

pytestmark = pytest.mark.gpu

TICKS, MISSED, S = 14, (6, 7), 4
OPTIONS = dict(slots=S, match_iou=0.3, max_age=2)
MOTION = dict(gain=1.0, decay=1.0)
BOXES, COUNTS = TC.table([[] if t in MISSED else [TC.box(4 + 6 * t, 30, 24)] for t in range(TICKS)], 2)


def test_a_walker_missed_for_two_ticks_keeps_one_identity_and_a_moving_crop(monkeypatch):
    plain = P.track_heads_host(BOXES, COUNTS, **OPTIONS)
    assert sorted(set(plain[2][plain[4] >= 0].tolist())) == [1, 2]                # what the option is for
    lg = live.LiveGaze(make_engine(), make_pipe(), cameras=1, clip_len=LC.CLIP, stride=LC.STRIDE, smooth=ALPHA, motion=MOTION, **OPTIONS)
    buf = torch.empty(*LC.FRAME_HW, 3, dtype=torch.uint8, device='cuda:0')
    frames = [dev(CAMS[0][t]) for t in range(TICKS)]
    tables = [(dev(BOXES[t][None]), dev(COUNTS[t][None])) for t in range(TICKS)]
    torch.cuda.synchronize()

    def refuse(*a, **k):
        raise AssertionError('the tick touched the host')

    ticks, results = [], []
    for t in range(TICKS):
        buf.copy_(frames[t])
        if t == 11:                                               # warmed up: a trunk call, a decoder call, a pop and the gate, with no host step
            for owner, name in ((torch.Tensor, 'cpu'), (torch.Tensor, 'item'), (torch.Tensor, 'tolist'), (torch.Tensor, 'numpy'), (torch.cuda, 'synchronize'),
                                (torch.cuda.Stream, 'synchronize'), (torch.cuda.Event, 'synchronize')):
                monkeypatch.setattr(owner, name, refuse)
        r = lg.tick([buf], *tables[t])
        monkeypatch.undo()
        ticks.append(dict(crop_boxes=lg.crop_boxes.clone(), image_of=lg.image_of.clone(), matched=r['matched'], flags=r['flags'], state=lg.state.clone()))
        results.append(r)
    results.append(lg.finish())
    torch.cuda.synchronize()
    assert results[11]['valid'].shape[0] == 1                     # the patched tick handed a frame out

    # the crop table of every tick is live_slots_host over the host tracker's state
    R = live.ring_depth(LC.CLIP)
    ring_id, ring_box = np.zeros((R, 1, S), np.int32), np.zeros((R, 1, S, 4), np.float32)
    state = None
    for t in range(TICKS):
        state = P.track_heads_host(BOXES[None, t:t + 1], COUNTS[None, t:t + 1], state=state, motion=MOTION, **OPTIONS)[6]
        crop_boxes, image_of, matched = live.live_slots_host(state, t, ring_id, ring_box)
        got = {k: v.cpu().numpy() for k, v in ticks[t].items()}
        same(got['state'], state, f'state, tick {t}')
        same(got['crop_boxes'], crop_boxes, f'crop_boxes, tick {t}')
        same(got['image_of'], image_of, f'image_of, tick {t}')
        same(got['matched'].reshape(matched.shape), matched, f'matched, tick {t}')
        assert crop_boxes[0].tolist() == [4.0 + 6 * t, 30.0, 28.0 + 6 * t, 54.0] and not crop_boxes[1:].any(), t      # where the person IS, seen or not
        assert got['flags'].tolist() == [0]

    track_id, valid = (torch.cat([r[name] for r in results]).cpu().numpy() for name in ('track_id', 'valid'))
    assert track_id.shape == (TICKS, 1, S)
    assert set(track_id[valid == 1].tolist()) == {1} and valid[:, 0, 0].all() and not valid[:, 0, 1:].any()           # one person, every frame valid
