"""Headless replay tracker: the reference's `track_points` + `track` loops (RealtimeTracking_FLIR.py:95-143, 157-209)
fed from recorded / synthetic frames instead of PySpin cameras, in batches through the HIP path.

What the reference does per time step, and what is kept here:
  * every camera thread runs `_find_dot` on its frame and queues the image points (:105-112);
  * `track` pairs the newest entries of the queues (:177-180), calls
    `find_point_correspondance_and_object_points(image_points, camera_poses, 4)` (:181) and sends
    `msgpack.packb({"tracker1": [0, 0, 0, 0, x, y, z]}, use_bin_type=True)` over TCP 127.0.0.1:5000 (:183-188); when
    no object point came out, the previous message is sent again (`point` keeps its value; it starts as eight zeros,
    :171).
Here frames of the same time step are paired by index (a recording has no queue races), the socket is the caller's
business (`send=` callback; networking is outside the path), and the message bytes are the reference's.
"""
import numpy as np
import torch

from .engine import GRAY_SHIFT, MocapContext
from .pipeline import BatchTracker

OBJ_COUNT = 4  # RealtimeTracking_FLIR.py:181


def tracker_message(point):
    """Wire format of one tracker update (RealtimeTracking_FLIR.py:186-187): msgpack map {"tracker1": point}."""
    import msgpack
    return msgpack.packb({"tracker1": [float(v) if isinstance(v, (float, np.floating)) else v for v in point]},
                         use_bin_type=True)


def unpack_tracker_message(data):
    import msgpack
    return msgpack.unpackb(data, raw=False)["tracker1"]


class ReplayTracker:
    """frames [T, C, H, W] (gray, or raw Bayer with `bayer_pattern`) -> per time step (object_points, image_points, message) exactly as `track` would produce
    them from the same detections.  `batch` time steps go through the GPU at once."""

    def __init__(self, K, dist, R, t, F, width, height, batch=64, obj_count=OBJ_COUNT, device=0, max_points=32,
                 max_groups=4096, bayer_pattern=None, gray_shift=GRAY_SHIFT, depth=1, visibility="all", min_views=2, gate=10.0,
                 max_err=25.0, max_passes=3, cutoff=10.0, max_hyp=8192, track=None, subpixel=None, bodies=None, refine=None):
        """visibility="any" (BatchTracker's): a time step yields the markers at least min_views cameras see, found from any
        camera pair, in acceptance order (more views first, then smaller error) -- the first obj_count + 1 of them as
        object_points, image_points [markers, C, 2] float64 with NaN where a camera does not see the marker; F may be None.
        depth > 1: that many batches are in flight on HIP streams of their own (BatchTracker's software pipelining): while
        the results of one batch are read back and turned into messages, the next ones are already on the GPU.  The time steps
        come out in order either way.
        track (BatchTracker's): marker identities across time steps and batches; the dicts of run_batches and run gain `ids` and
        `ages`, row for row beside object_points (-1 = the row's marker got no track).  The black frames that pad the last batch
        are not walked: they do not age the tracks.  The messages stay as they are.
        subpixel (BatchTracker's): {"radius": r, "floor": f, "iters": 3} -- the object points are triangulated from sub-pixel image
        points; image_points keep their integer form (visibility="any": the records' centroids; "all": the refined points, truncated).
        bodies (BatchTracker's): {"models": [...], "tol": ..., "gate": ..., "min_markers": 3, "names": [...]} -- rigid-body poses
        per time step; the dicts of run_batches gain body_R, body_t, body_q, body_rms, body_n, body_label, body_status (host
        arrays [n_steps, B, ...]) and body_messages: per time step one rigid_message per body, {"<name>": [w, x, y, z, tx, ty, tz]};
        a body without a pose in a step repeats its previous message (seven zeros until its first pose).  run() yields the same per
        time step.  The labels are rows of the step's markers before the obj_count selection.  `messages` stay as they are.
        refine (BatchTracker's): {"max_iters": 10, "ftol": 1e-9, "lambda0": 1e-3, "max_res2": ..., "max_drop": 0} -- the markers are
        moved to the minimum of their reprojection error: object_points, and with them the messages, hold the refined points
        (`track` and `bodies` read them too; a marker that could not be refined keeps its point).  None is the path as it was."""
        self.n_cam = len(K)
        self.batch = int(batch)
        self.obj_count = obj_count
        self.width, self.height = width, height
        self.depth = max(1, int(depth))
        self.tracker = BatchTracker(K, dist, R, t, F, width, height, self.batch, device=device, max_points=max_points,
                                    max_groups=max_groups, bayer_pattern=bayer_pattern, gray_shift=gray_shift, depth=self.depth,
                                    visibility=visibility, min_views=min_views, gate=gate, max_err=max_err, max_passes=max_passes,
                                    cutoff=cutoff, max_hyp=max_hyp, track=track, subpixel=subpixel, bodies=bodies, refine=refine)
        self.visibility = visibility
        self.refined = refine is not None
        self.tracked = track is not None
        self.body_names = self.tracker.body_tables["names"] if bodies is not None else None
        if self.body_names is not None:  # the message in force per body: zeros until its first pose
            self.body_carry = [rigid_message(name, [0.0] * 4, [0.0] * 3) for name in self.body_names]
        self.point = [0, 0, 0, 0, 0, 0, 0, 0]  # RealtimeTracking_FLIR.py:171 (eight zeros until the first detection)
        # raw sensor frames: the camera loop's cvtColor(BAYER_GR2BGR) + cvtColor(BGR2GRAY) (:103-104) run on the GPU first, with
        # no gray frame in memory (BatchTracker.extract); bayer_pattern 0..3 = BG, GB, RG, GR (the reference: 3), None = the
        # frames are gray already
        self.bayer_pattern, self.gray_shift = bayer_pattern, gray_shift

    def _select(self, xyz, order, n):
        idx = order[:n]
        if not self.obj_count > len(idx):  # lib/Helpers.py:275-278
            idx = idx[: self.obj_count + 1]
        return xyz[idx]

    def _submit(self, frames):
        """Generator over the batches of `frames` (one array / tensor [T, C, H, W], or a list of such pieces), each submitted to the
        GPU: (first time step, time steps, outputs), at most `depth` of them in flight, oldest first."""
        dev = self.tracker.ctx.device
        pending = []  # batches submitted and not yet read back; at most depth - 1 wait here
        parts = frames if isinstance(frames, (list, tuple)) else [frames]  # a recording in several pieces: one after the other
        t_base = 0
        for part in parts:
            assert part.shape[1:] == (self.n_cam, self.height, self.width), part.shape
            for p0 in range(0, part.shape[0], self.batch):
                chunk = part[p0:p0 + self.batch]
                nb = chunk.shape[0]
                if isinstance(chunk, np.ndarray):
                    chunk = torch.from_numpy(np.ascontiguousarray(chunk))
                # depth 1: the plain blocking copy.  Deeper pipelines upload asynchronously (a pinned caller tensor is then read
                # later: the caller must leave that piece of the frames untouched until the batch's results have been yielded)
                chunk = chunk.to(dev, non_blocking=self.depth > 1)
                if nb < self.batch:  # pad the last batch with black frames (they produce no points)
                    pad = torch.zeros((self.batch - nb,) + tuple(chunk.shape[1:]), dtype=torch.uint8, device=dev)
                    chunk = torch.cat([chunk, pad], dim=0)
                out = self.tracker.step(chunk.reshape(self.batch * self.n_cam, self.height, self.width).contiguous(),
                                        steps=nb if self.tracked else None)
                pending.append((t_base + p0, nb, out))
                if len(pending) >= self.depth:  # the oldest batch's lane is the next one to be reused: read it back first
                    yield pending.pop(0)
            t_base += part.shape[0]
        while pending:
            yield pending.pop(0)

    def _collect(self, b0, nb, out):
        """One batch read back (one device-to-host copy per output) and turned into what `track` produces, for all of its time
        steps at once: the `obj_count + 1` selection of lib/Helpers.py:274-279, the image points, and the message bytes -- built
        in bulk (batch_messages), the previous message repeated for time steps without a point (RealtimeTracking_FLIR.py:181-188)."""
        n = self.tracker.finish(out, first_step=b0)[:nb]  # raises CapacityError: no time step is answered from shortened lists
        if self.visibility == "any":
            return self._collect_any(b0, nb, out, n)
        xyz = out["xyz_refined" if self.refined else "xyz"].cpu().numpy()[:nb]
        grp = out["grp"].cpu().numpy()[:nb].astype(np.int64)
        order = out["order"].cpu().numpy()[:nb]
        oc = self.obj_count
        kept = np.where(n >= oc, np.minimum(n, oc + 1), n)  # `if not obj_count > len(...)`: lib/Helpers.py:275-278
        width = min(oc + 1, xyz.shape[1])
        sel = np.clip(order[:, :width], 0, xyz.shape[1] - 1)
        obj = xyz[np.arange(nb)[:, None], sel]  # [nb, <= obj_count + 1, 3]; rows beyond kept[s] are not results
        has = kept > 0
        msgs = batch_messages(obj[:, 0] if width else np.zeros((nb, 3)), has, tracker_message(self.point))
        if has.any():
            self.point = [0, 0, 0, 0] + list(obj[np.flatnonzero(has)[-1], 0])  # :184-185
        res = {"first_step": b0, "n_steps": nb, "n_roots": n, "kept": kept, "object_points": obj, "image_points": grp, "messages": msgs}
        return self._with_bodies(self._with_ids(res, out, n, width), out)

    def _with_bodies(self, res, out):
        """body_* [n_steps, B, ...] and body_messages: one device-to-host copy per output, the messages built in bulk per body"""
        if self.body_names is None:
            return res
        nb = res["n_steps"]
        for key in BatchTracker.BODY_KEYS.values():
            res[key] = out[key].cpu().numpy()[:nb]
        has = res["body_status"] == 0
        per_body = []
        for b, name in enumerate(self.body_names):
            q = np.where(has[:, b, None], res["body_q"][:, b], 0.0)  # (the floats of a step without a pose are not read)
            t = np.where(has[:, b, None], res["body_t"][:, b], 0.0)
            msgs = batch_rigid_messages(name, q, t, has[:, b], self.body_carry[b])
            if nb:
                self.body_carry[b] = msgs[-1]
            per_body.append(msgs)
        res["body_messages"] = [[per_body[b][s] for b in range(len(self.body_names))] for s in range(nb)]
        return res

    def _with_ids(self, res, out, n, width):
        """ids / ages [n_steps, width] beside object_points (the tracker's rows are object_points' rows in both visibilities)"""
        if self.tracked:
            nb = res["n_steps"]
            live = np.arange(width)[None, :] < n[:, None]
            for name, key in (("ids", "id"), ("ages", "age")):
                res[name] = np.where(live, out[key].cpu().numpy()[:nb, :width], -1)
        return res

    def _collect_any(self, b0, nb, out, n):
        """_collect for visibility="any": the rows below n[s] are the markers, already in their order; nothing beyond them is
        read (mocap_correspond_visible leaves those rows unspecified)."""
        lane = next(l for l in self.tracker.lanes if l.out is out)
        xyz = out["xyz_refined" if self.refined else "xyz"].cpu().numpy()[:nb]
        idx = out["idx"].cpu().numpy()[:nb]
        xy, _ = MocapContext.record_views(lane.records)
        xy = xy.cpu().numpy().reshape(self.batch, self.n_cam, -1, 2)[:nb]
        Q = xyz.shape[1]
        live = np.arange(Q)[None, :] < n[:, None]                     # [nb, Q]: the row holds a marker
        oc = self.obj_count
        kept = np.where(n >= oc, np.minimum(n, oc + 1), n)
        width = min(oc + 1, Q)
        obj = np.where(live[:, :width, None], xyz[:, :width], 0.0)   # sliced by n before anything else looks at it
        member = live[:, :, None] & (idx >= 0)                        # [nb, Q, C]
        pick = np.where(member, idx, 0)
        img = xy[np.arange(nb)[:, None, None], np.arange(self.n_cam)[None, None, :], pick].astype(np.float64)  # [nb, Q, C, 2]
        img[~member] = np.nan
        has = kept > 0
        msgs = batch_messages(obj[:, 0], has, tracker_message(self.point))
        if has.any():
            self.point = [0, 0, 0, 0] + list(obj[np.flatnonzero(has)[-1], 0])
        res = {"first_step": b0, "n_steps": nb, "n_roots": n, "kept": kept, "object_points": obj, "image_points": img, "messages": msgs}
        return self._with_bodies(self._with_ids(res, out, n, width), out)

    def run_batches(self, frames, send_many=None):
        """Generator over BATCHES of time steps: dicts with first_step, n_steps, n_roots [n], kept [n] (object points per time
        step), object_points [n, <= obj_count + 1, 3] (rows beyond kept[s] unused), image_points [n, P, C, 2] int64 (rows
        beyond n_roots[s] unused), messages (list of n bytes objects); with `track`, ids and ages [n, <= obj_count + 1] int32 beside
        object_points.  `send_many(list_of_bytes)` is called once per batch when
        given.  The bulk form of run(): no Python work per time step."""
        for b0, nb, out in self._submit(frames):
            res = self._collect(b0, nb, out)
            if send_many is not None:
                send_many(res["messages"])
            yield res

    def learn_bodies(self, frames, *, spread, min_steps, **kw):
        """Rigid-body models learned from a take (MocapContext.learn_rigid_bodies, whose keywords `kw` are): the frames run
        through the tracker, which must have been built with `track`; per batch the marker rows that `track` read, their counts
        and their identities are kept on the device, for the real time steps only -- the black frames that pad the last batch
        are not included -- and the whole take is handed over at once.  Returns learn_rigid_bodies' dict: its `models` are ready
        for bodies={"models": ...}.  Use a tracker that has seen nothing else: the identities continue from its state."""
        if not self.tracked:
            raise ValueError("learn_bodies needs the marker identities: build the tracker with track={'gate': ...}")
        xyz, n, ids = [], [], []
        for b0, nb, out in self._submit(frames):
            self.tracker.finish(out, first_step=b0)  # raises CapacityError: no model is learned from shortened lists
            xyz.append(self.tracker._marker_rows(out)[:nb].clone())
            n.append(out["n"][:nb].clone())
            ids.append(out["id"][:nb].clone())
        if not xyz:
            raise ValueError("learn_bodies: the take has no frames")
        return self.tracker.ctx.learn_rigid_bodies(torch.cat(xyz).contiguous(), torch.cat(n).contiguous(), torch.cat(ids).contiguous(),
                                                   spread=spread, min_steps=min_steps, **kw)

    def run(self, frames, send=None):
        """Generator over time steps.  frames: uint8 [T, C, H, W] NumPy array or torch tensor (host or device).
        Yields dicts: object_points [<= obj_count+1, 3] (or shape (0,)), image_points [roots, C, 2] (or (0,)),
        message (bytes); with `track`, ids and ages [<= obj_count+1] beside object_points.  `send(bytes)` is called per time step when given."""
        empty = np.array([])
        none = np.array([], np.int32)
        for res in self.run_batches(frames):
            n, kept, obj, img, msgs = res["n_roots"], res["kept"], res["object_points"], res["image_points"], res["messages"]
            for s in range(res["n_steps"]):
                if send is not None:
                    send(msgs[s])
                k = int(n[s])
                one = {"object_points": obj[s, :kept[s]] if k else empty, "image_points": img[s, :k] if k else empty, "message": msgs[s]}
                if self.tracked:
                    one["ids"], one["ages"] = (res[f][s, :kept[s]] if k else none for f in ("ids", "ages"))
                if self.body_names is not None:
                    for key in list(BatchTracker.BODY_KEYS.values()) + ["body_messages"]:
                        one[key] = res[key][s]
                yield one


def rigid_message(name, q, t):
    """Wire format of one rigid-body update: msgpack map {"<name>": [w, x, y, z, tx, ty, tz]}, seven float64 -- the reference's
    tracker message with its four orientation slots (scalar first, as its IMU code has them) filled."""
    import msgpack
    return msgpack.packb({str(name): [float(v) for v in list(q) + list(t)]}, use_bin_type=True)


def unpack_rigid_message(data):
    """-> (name, q [4], t [3])"""
    import msgpack
    (name, v), = msgpack.unpackb(data, raw=False).items()
    return name, v[:4], v[4:]


def _rigid_head(name):
    raw = str(name).encode("utf-8")
    if len(raw) < 32:
        key = bytes([0xa0 | len(raw)])            # fixstr
    elif len(raw) < 256:
        key = bytes([0xd9, len(raw)])             # str 8
    else:
        raise ValueError(f"a body name of {len(raw)} bytes: at most 255")
    return bytes([0x81]) + key + raw + bytes([0x97])  # map of 1, the key, array of 7


def batch_rigid_messages(name, q, t, has, carry):
    """The rigid_message bytes of one body over a run of time steps, built without a Python loop over them (batch_messages' way):
    q [n, 4], t [n, 3] float64, has [n] bool (the step has a pose), carry: the message in force before the run."""
    n = len(has)
    head = _rigid_head(name)
    L = len(head) + 63
    buf = np.empty((n, L), np.uint8)
    buf[:, :len(head)] = np.frombuffer(head, np.uint8)
    body = buf[:, len(head):].reshape(n, 7, 9)
    body[:, :, 0] = 0xcb
    vals = np.concatenate([np.asarray(q, np.float64).reshape(n, 4), np.asarray(t, np.float64).reshape(n, 3)], axis=1)
    body[:, :, 1:] = np.ascontiguousarray(vals).astype(">f8").view(np.uint8).reshape(n, 7, 8)
    src = np.maximum.accumulate(np.where(has, np.arange(n), -1)) if n else np.zeros(0, np.int64)
    raw = buf[np.maximum(src, 0)].tobytes()
    return [raw[i * L:(i + 1) * L] if src[i] >= 0 else carry for i in range(n)]


_MSG_HEAD = bytes([0x81, 0xa8]) + b"tracker1" + bytes([0x97, 0, 0, 0, 0])  # map of 1, fixstr(8), array of 7, four zero ints


def batch_messages(first_points, has, carry):
    """The tracker messages of a run of time steps, built without a Python loop over them.  first_points [n, 3] float64 (the
    first object point of each time step), has [n] bool (the time step produced a point), carry: the message in force before
    the run.  Returns a list of n bytes objects: msgpack.packb({"tracker1": [0, 0, 0, 0, x, y, z]}, use_bin_type=True) for a
    time step with a point (a map of one entry, fixstr key, array of seven: four zero fixints and three float64, big endian),
    else the message of the last time step that had one (`point` keeps its value, RealtimeTracking_FLIR.py:181-188)."""
    n = len(has)
    L = len(_MSG_HEAD) + 27
    buf = np.empty((n, L), np.uint8)
    buf[:, :len(_MSG_HEAD)] = np.frombuffer(_MSG_HEAD, np.uint8)
    body = buf[:, len(_MSG_HEAD):].reshape(n, 3, 9)
    body[:, :, 0] = 0xcb
    body[:, :, 1:] = np.ascontiguousarray(first_points, np.float64).astype(">f8").view(np.uint8).reshape(n, 3, 8)
    src = np.maximum.accumulate(np.where(has, np.arange(n), -1))  # the time step whose message is in force
    raw = buf[np.maximum(src, 0)].tobytes()
    return [raw[i * L:(i + 1) * L] if src[i] >= 0 else carry for i in range(n)]


__all__ = ["ReplayTracker", "batch_messages", "tracker_message", "unpack_tracker_message", "rigid_message", "unpack_rigid_message",
           "batch_rigid_messages", "OBJ_COUNT", "MocapContext"]
