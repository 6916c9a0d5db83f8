"""LiveGaze(draw=True, labels=...) and run_head_video(draw=dict(labels=...)) on the device: the frames handed out are
arrows.draw_labels_host over the frames a run WITHOUT labels hands out and the tables the call itself returns, every other table is bit-equal
to that run, the tick still never waits for the device, and labels without draw (or region_names without regions) is refused.  The scene, the
frames and the engine are those of tests/test_gpu_live_attention_poly.py."""
import numpy as np
import pytest
import torch

from mcgaze_amd import arrows as AR
from mcgaze_amd import attention as AT
from mcgaze_amd import harness, live
from tests import labels_cases as LB
from tests import live_cases as LC
from tests import overlay_cases as O
from tests.live_gpu_common import ALPHA, CAMS, DEV, H, W, dev, make_engine, make_pipe, same
from tests.test_gpu_live_attention_poly import MIXED, OPTIONS, TICKS, TRAPEZOID

pytestmark = pytest.mark.gpu

NAMES = [['DESK', None], ['SHELF A']]                             # per camera: MIXED has two regions on camera 0, one on camera 1
FPS = (30000, 1001)
# (attention, overlay, dwell, region_names, scale): everything at once; labels alone in the arrow's colour; names and dwell without the overlay
VARIANTS = dict(all=(True, True, True, True, 1), plain=(False, False, False, False, 2), names=(True, False, True, True, 1))


@pytest.fixture(scope='module')
def engine():
    return make_engine()


@pytest.fixture(scope='module')
def pipe():
    return make_pipe()


def options(variant, labels):
    attention, overlay, dwell, names, scale = VARIANTS[variant]
    kw = dict(draw=True)
    if attention:
        kw.update(attention=dict(OPTIONS, regions=MIXED))
    if overlay:
        kw.update(overlay=dict(palette=O.PALETTE, line_thickness=3, region_thickness=1))
    if dwell:
        kw.update(dwell=True)
    if labels:
        kw.update(labels=dict(scale=scale, fps=FPS, background=(40, 30, 20), region_names=NAMES if names else None))
    return kw


def run(engine, pipe, lanes, **kw):
    boxes, counts = LC.scene()
    lg = live.LiveGaze(engine, pipe, cameras=LC.Q, clip_len=LC.CLIP, stride=LC.STRIDE, smooth=ALPHA, lanes=lanes, **kw, **LC.OPTIONS)
    bufs = [torch.empty(H, W, 3, dtype=torch.uint8, device=DEV) for _ in range(LC.Q)]
    results = []
    for t in range(TICKS):
        for q in range(LC.Q):
            bufs[q].copy_(dev(CAMS[q][t]))
        results.append(lg.tick(bufs, dev(boxes[t]), dev(counts[t])))
    results.append(lg.finish())
    torch.cuda.synchronize()
    host = lambda v: v.cpu().numpy() if isinstance(v, torch.Tensor) else v
    return [{k: [[host(f) for f in fr] for fr in v] if k == 'frames' else host(v) for k, v in r.items()} for r in results]


@pytest.mark.parametrize('variant', list(VARIANTS))
@pytest.mark.parametrize('lanes', [None, 3], ids=['slots', 'lanes'])
def test_live_frames_are_the_twin_over_the_returned_tables_and_the_tables_do_not_change(engine, pipe, lanes, variant):
    attention, overlay, dwell, names, scale = VARIANTS[variant]
    got, plain = run(engine, pipe, lanes, **options(variant, True)), run(engine, pipe, lanes, **options(variant, False))
    if names:
        regions, region_image, _ = AT._attention_options('LiveGaze', dict(regions=MIXED), LC.Q)
        rb, rio, rtext, rplace = AT.region_label_rows(regions, region_image, [s for c in NAMES for s in c], LC.Q, region_period=LC.Q)
        assert rio.tolist() == [0, 1]
    else:
        rb, rio, rtext, rplace = np.zeros((0, 4), np.float32), np.zeros(0, np.int32), np.zeros((0, 24), np.uint8), np.zeros(0, np.int32)
    pal = np.asarray(O.PALETTE if overlay else AR.OVERLAY_PALETTE, np.uint8)
    words = changed = 0
    for r, p in zip(got, plain):
        assert set(r) == set(p) and r['first'] == p['first']
        for name in p:
            if name not in ('first', 'frames'):
                same(r[name], p[name], name)                      # every other table is bit-equal to the run without labels
        k = r['valid'].shape[0]
        assert len(r['frames']) == k
        for i in range(k):
            n = r['track_id'][i].size
            ids = np.where(r['valid'][i] != 0, r['track_id'][i], 0).reshape(-1)
            text = AR.format_labels_host(ids, r['dwell_frames'][i].reshape(-1) if dwell else None, FPS)
            image_of = r['image_of'][i].reshape(-1)
            image_of = np.where(image_of >= 0, image_of - i * LC.Q, image_of)
            ok = image_of >= 0                                    # an invalid row is not drawn on the device (flag 2); the twin leaves it out
            if overlay:
                kind, mutual = r['target_kind'][i].reshape(-1), r['mutual'][i].reshape(-1)
                row_colors = pal[np.where(mutual != 0, 4, np.where((kind >= 1) & (kind <= 3), kind, 0))]
            else:
                row_colors = np.tile(pal[0], (n, 1))
            colors = np.concatenate([np.tile(pal[5], (len(rb), 1)), row_colors[ok]]).astype(np.uint8)
            want, flags = AR.draw_labels_host(p['frames'][i], np.concatenate([rb, r['head_box'][i].reshape(-1, 4)[ok]]), np.concatenate([rio, image_of[ok]]),
                                              np.concatenate([rtext, text[ok]]), colors=colors, background=(40, 30, 20), scale=scale,
                                              place=np.concatenate([rplace, np.zeros(int(ok.sum()), np.int32)]))
            assert not (flags == 2).any()
            LB.same('bgr', r['frames'][i], want, (r['first'], i))
            words += int((flags[len(rb):] == 0).sum())
            assert all(bytes(t).startswith(b'#') for t in text[ok][flags[len(rb):] == 0])
            if dwell:
                assert all(b's' in bytes(t) for t, f in zip(text, r['dwell_frames'][i].reshape(-1)) if f > 0 and t[0])
            changed += sum(not np.array_equal(a, b) for a, b in zip(r['frames'][i], p['frames'][i]))
    assert words > 0 and changed > 0


def test_a_tick_with_labels_never_waits_for_the_device(engine, pipe, monkeypatch):
    boxes, counts = LC.scene()
    lg = live.LiveGaze(engine, pipe, cameras=LC.Q, clip_len=LC.CLIP, stride=LC.STRIDE, smooth=ALPHA, **options('all', True), **LC.OPTIONS)
    bufs = [dev(CAMS[0][0]), dev(CAMS[1][0])]
    tables = [(dev(boxes[t]), dev(counts[t])) for t in range(12)]
    for t in range(11):
        lg.tick(bufs, *tables[t])
    torch.cuda.synchronize()

    def refuse(*a, **k):
        raise AssertionError('the tick touched the host')

    def only_if_complete(event):
        # draw=True brings the table of the fresh frame copies up through the staging ring (with or without labels), and a stage that is
        # taken again asks for the event of the copy it made four uploads earlier.  That is no wait iff the copy is over: the tick may ask
        # only about events that are already complete.
        assert event.query(), 'the tick waited for the device'

    for owner, name in ((torch.Tensor, 'cpu'), (torch.Tensor, 'item'), (torch.Tensor, 'tolist'), (torch.Tensor, 'numpy'), (torch.cuda, 'synchronize'),
                        (torch.cuda.Stream, 'synchronize')):
        monkeypatch.setattr(owner, name, refuse)
    monkeypatch.setattr(torch.cuda.Event, 'synchronize', only_if_complete)
    r = lg.tick(bufs, *tables[11])                                # tick 11 returns frame 3: the gate, the targets, dwell, the overlay, the labels
    monkeypatch.undo()
    torch.cuda.synchronize()
    assert r['first'] == 3 and len(r['frames']) == 1 and r['valid'][0, 0, 0].item() == 1
    assert bytes(lg.label_text[lg.label_regions].cpu().numpy()).startswith(b'#')      # the first row label, behind the region rows


def test_labels_need_draw_and_region_names_need_regions(engine, pipe):
    kw = dict(cameras=LC.Q, clip_len=LC.CLIP, stride=LC.STRIDE, **LC.OPTIONS)
    for bad in (dict(labels=True), dict(labels=dict(scale=2)), dict(labels=dict(size=2), draw=True), dict(labels=dict(scale=17), draw=True),
                dict(labels=dict(fps=(1, 2)), draw=True), dict(labels=3, draw=True), dict(labels=dict(region_names=NAMES), draw=True),
                dict(labels=dict(region_names=NAMES[:1]), draw=True, attention=dict(regions=MIXED)),
                dict(labels=dict(region_names=[['a'], ['b']]), draw=True, attention=dict(regions=MIXED))):
        with pytest.raises(ValueError):
            live.LiveGaze(engine, pipe, **kw, **bad)
    frames = [CAMS[0][t] for t in range(3)]
    with pytest.raises(ValueError):
        harness.run_head_video(engine, pipe, frames, [[[10, 20, 40, 56]]] * 3, max_len=4, draw=dict(labels=dict(scale=0)))
    with pytest.raises(ValueError):
        harness.run_head_video(engine, pipe, frames, [[[10, 20, 40, 56]]] * 3, max_len=4, draw=dict(labels=dict(region_names=[['a']])))


def test_run_head_video_labels_its_own_records(engine, pipe):
    frames = [CAMS[0][t] for t in range(9)]
    per_frame = [[[10 + t, 20, 40 + t, 56], [80, 24, 112, 60]] for t in range(6)] + [[[30, 20, 62, 58]] for _ in range(3)]
    attention = dict(regions=[[100, 0, W, 40], TRAPEZOID], expand=0.5)
    for more, label_kw in ((dict(), True), (dict(attention=attention, dwell=True), dict(scale=1, fps=FPS, background=None))):
        plain, drawn = harness.run_head_video(engine, pipe, frames, per_frame, max_len=4, smooth=ALPHA, draw=dict(min_thickness=2), **more)
        records, annotated = harness.run_head_video(engine, pipe, frames, per_frame, max_len=4, smooth=ALPHA, draw=dict(min_thickness=2, labels=label_kw), **more)
        torch.cuda.synchronize()
        assert len(annotated) == 9 and len(records) == len(plain)
        for g, r in zip(records, plain):                          # the records are those of the run without labels
            assert sorted(g) == sorted(r)
            for k in r:
                assert np.array_equal(g[k], r[k]) if isinstance(r[k], np.ndarray) else g[k] == r[k], k
        opts = dict(scale=2, background=(0, 0, 0)) if label_kw is True else dict(scale=1, background=None)
        for t in range(9):
            here = [(number, r, r['frame_id'].index(t)) for number, r in enumerate(records) if t in r['frame_id']]
            ids = [r['id'] if isinstance(r['id'], (int, np.integer)) else number + 1 for number, r, _ in here]
            values = [int(r['dwell_frames'][j]) for _, r, j in here] if more else None
            text = AR.format_labels_host(ids, values, FPS if more else (30, 1))
            want, flags = AR.draw_labels_host(drawn[t].cpu().numpy(), np.stack([r['head_box'][j] for _, r, j in here]), None, text, **opts)
            assert flags.tolist() == [0] * len(here)
            assert np.array_equal(annotated[t].cpu().numpy(), want) and not np.array_equal(want, drawn[t].cpu().numpy()), t
