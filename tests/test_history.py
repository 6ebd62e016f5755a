"""Frame history on the CPU backend: a camera added with history H keeps its H newest decoded
frames readable (Worker.read_history) and a job of several pictures publishes its last H outputs,
not only the newest.

Reference semantics: the worker XADDs every frame it decodes into a Redis stream capped at
``buffer.in_memory`` entries (python/read_image.py:87-121), so after a lazy-decode catch-up a
consumer sees every picture of the GOP up to now.

The lazy catch-up: the issue words it as 13 silent access units and then one more with gop=12.
Access unit 12 of that stream is the next IDR, which restarts the camera's GOP buffer
(Camera::on_access_unit), so a query at access unit 13 catches up over two pictures only. The
catch-up over "the whole GOP" it asks for is the query arriving at the GOP's last access unit:
11 silent access units, then one more.
"""
import numpy as np
import pytest

from history_util import avc_stream, check_window, hevc_stream, now_ms

H = 5


@pytest.fixture(scope="module")
def avc(native):
    return avc_stream(native, 20)


@pytest.fixture(scope="module")
def hevc(native):
    return hevc_stream(native, 14)


@pytest.fixture
def live(native):
    w = native.Worker(device=-1)
    w.start()
    yield w
    w.stop()


def catch_up(w, cam, aus, n):
    """n - 1 access units nobody watches, then a query and one more: one job for all of them."""
    for au in aus[:n - 1]:
        assert w.submit_au(cam, au) is False
    w.flush()
    assert w.stats(cam)["published"] == 0
    w.set_last_query(cam, now_ms())
    assert w.submit_au(cam, aus[n - 1])
    w.flush()


def test_lazy_catch_up_publishes_the_newest_outputs(native, live, avc):
    aus, outs, upto = avc
    cam = live.add_camera("catchup", 2, H)
    assert upto[11] >= 6, "the reference alone must have more outputs than the history holds"
    catch_up(live, cam, aus, 12)
    want = outs[:upto[11]][-H:]
    frames = live.read_history(cam)
    assert len(frames) == H
    check_window(frames, want)
    assert [m["seq"] for m, _ in frames] == [1, 2, 3, 4, 5]
    meta, newest = live.read_latest(cam, 0)
    assert meta["seq"] == 5 and meta["pts"] == want[-1][0] and np.array_equal(newest, want[-1][3])
    st = live.stats(cam)
    assert st["history"] == H and st["published"] == H and st["decoded"] == H
    assert st["history_skipped"] == upto[11] - H  # the older outputs of the job
    assert st["ring_slots"] >= live.history_ring_slots(H) == 2 * H


def test_history_off_publishes_one_frame(native, live, avc):
    aus, outs, upto = avc
    cam = live.add_camera("plain", 2)  # history 0, as before
    catch_up(live, cam, aus, 12)
    st = live.stats(cam)
    assert st["published"] == 1 and st["decoded"] == 1 and st["history"] == 0 and st["history_skipped"] == 0
    frames = live.read_history(cam)
    assert len(frames) == 1
    check_window(frames, outs[:upto[11]][-1:])
    assert live.read_history(cam, 0, 4)[0][0]["seq"] == 1 and len(live.read_history(cam, 0, 4)) == 1


@pytest.mark.parametrize("codec", ["h264", "h265"])
def test_decode_many_merges_every_output(native, codec, avc, hevc):
    """merge_job: the access units of one decode_many call become one job; its outputs append."""
    aus, outs, upto = avc if codec == "h264" else hevc
    w = native.Worker(device=-1)
    cam = w.add_camera("many", 2, H)
    n = 12
    assert upto[n - 1] >= 6
    assert w.decode_many([(cam, aus[:n])]) == 1
    frames = w.read_history(cam)
    assert len(frames) == H
    check_window(frames, outs[:upto[n - 1]][-H:])
    assert w.stats(cam)["published"] == H
    meta, newest = w.read_latest(cam, 0)
    assert meta["pts"] == outs[upto[n - 1] - 1][0] and np.array_equal(newest, outs[upto[n - 1] - 1][3])


def test_cursor_and_count(native, avc):
    aus, outs, upto = avc
    w = native.Worker(device=-1)
    cam = w.add_camera("cursor", 2, H)
    w.decode_many([(cam, aus[:12])])
    want = outs[:upto[11]][-H:]
    after = w.read_history(cam, 3)
    assert [m["seq"] for m, _ in after] == [4, 5]
    check_window(after, want[3:])
    assert w.read_history(cam, 5) == []
    two = w.read_history(cam, 0, 2)  # a count below H: the newest `count`
    assert [m["seq"] for m, _ in two] == [4, 5]
    check_window(two, want[3:])
    assert [m["seq"] for m, _ in w.read_history(cam, 0, 50)] == [1, 2, 3, 4, 5]  # never more than H
    assert w.history_seqs(cam) == [1, 2, 3, 4, 5] and w.history_seqs(cam, 3) == [4, 5]
    vf = w.video_frames(cam, 3, 0, "cursor")
    assert [s for s, _ in vf] == [4, 5] and all(isinstance(b, bytes) and len(b) > 176 * 144 * 3 for _, b in vf)


def test_frames_survive_later_jobs(native, avc):
    """Retention: a following single-picture job slides the window by exactly one frame."""
    aus, outs, upto = avc
    w = native.Worker(device=-1)
    cam = w.add_camera("retain", 2, H)
    w.decode_many([(cam, aus[:11])])
    k = upto[10]
    check_window(w.read_history(cam), outs[:k][-H:])
    first = w.read_history(cam)[0][0]["seq"]
    for i in (11, 12, 13, 14):  # (access unit 12 is the next IDR)
        assert upto[i] == upto[i - 1] + 1, "this stream outputs one frame per access unit"
        assert w.decode_now(cam, aus[i])
        frames = w.read_history(cam)
        assert len(frames) == H and frames[0][0]["seq"] == first + (i - 10)
        check_window(frames, outs[:upto[i]][-H:])
    assert w.stats(cam)["published"] == first + H - 1 + 4


def test_stale_outputs_of_a_keyframe_restart_are_not_committed(native, avc):
    """A backlog that reaches a keyframe restarts from it (merge_job): the outputs the restarted
    job releases were reconstructed by the pictures it dropped, so none of them enters the
    history; frames committed before stay, and the stream picks up after the restart."""
    aus, outs, upto = avc
    w = native.Worker(device=-1)
    cam = w.add_camera("restart", 2, H)
    w.decode_many([(cam, aus[:6])])
    before = w.read_history(cam)
    check_window(before, outs[:upto[5]][-H:])
    pub = w.stats(cam)["published"]
    assert pub == min(H, upto[5]) and pub >= 2
    # access units 6 .. 13: the IDR at 12 drops 6 .. 11; 12 and 13 release pictures of those
    w.decode_many([(cam, aus[6:14])])
    st = w.stats(cam)
    assert st["published"] == pub, "a stale output of the restarted job was committed"
    assert st["errors"] == 0
    kept = w.read_history(cam)
    assert [m["seq"] for m, _ in kept] == [m["seq"] for m, _ in before]
    check_window(kept, outs[:upto[5]][-H:])
    # the new GOP's pictures are published as they leave the reorder buffer
    new = []
    for i in range(14, 20):
        w.decode_now(cam, aus[i])
    frames = w.read_history(cam)
    new = [m["pts"] for m, _ in frames if m["seq"] > pub]
    assert new and new == sorted(new) and min(new) >= aus[12].pts
    by_pts = {o[0]: o for o in outs}
    check_window([f for f in frames if f[0]["seq"] > pub], [by_pts[p] for p in new])


def test_ring_never_hands_out_a_retained_slot(native, avc):
    """Many jobs on the smallest ring a history camera gets: every read is a contiguous run of the
    H newest frames with the right pixels (a reused retained slot would break one of them)."""
    aus, outs, upto = avc
    w = native.Worker(device=-1)
    cam = w.add_camera("ring", 1, 3)
    assert w.stats(cam)["ring_slots"] == w.history_ring_slots(3)
    by_pts = {o[0]: o for o in outs}
    for i, au in enumerate(aus):
        w.decode_now(cam, au)
        frames = w.read_history(cam)
        pub = w.stats(cam)["published"]
        assert pub == upto[i] and len(frames) == min(3, pub)
        if frames:
            assert frames[-1][0]["seq"] == pub
            check_window(frames, [by_pts[m["pts"]] for m, _ in frames])
