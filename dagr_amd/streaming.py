"""Event streams: detections on a sliding window that is kept on the device.

The engine detects on a window (``model(x, reset=True)``) and can attach events to one (``reset=False``); an
``EventStream`` moves the window forward.  The raw events of the running window stay in device memory; a step uploads the
NEW events only, two launches (``dagr_stream_stage``) retire what has left the window and write the next window into the
static input buffers of the engine's captured window, and the window replays unchanged.  The host does no cutting, no
``format_data`` and does not learn the window's size.

What a step computes -- the definition, which ``StreamDefinition`` below states once in numpy (the yardstick of the
documentation and of the tests; nothing on the device path calls it):

* lanes ``b = 0 .. B-1`` are the samples of the model's ``batch_size``; each lane is an endless sequence of events
  ``(x, y)`` int16 pixels, ``t`` int64 absolute microseconds, ``p`` int8 in {-1, +1}; inside a lane ``t`` is
  non-decreasing, within a push and across pushes;
* after a push ``t_ref[b]`` is ``t_now[b]`` when the caller gives ``t_now``, else the ``t`` of the lane's newest event;
  it must not be older than the lane's newest event nor than the lane's previous ``t_ref``;
* the lane's window is every event ever pushed to it with ``0 <= t_ref[b] - t < window_us``, in arrival order (a suffix of
  the lane: what has left never comes back);
* ``t_rel = time_window - (t_ref[b] - t)`` as int32 -- without ``t_now`` the newest event sits at ``time_window``, where
  ``DSEC.preprocess_events`` puts it (data/dsec_data.py:157-163); ``window_us <= time_window``;
* the batch window is the lanes' windows concatenated in lane order, the model input is ``format_data`` of
  ``(x, y, t_rel, p)`` under the engine's ``(W, H, time_window)``, and the step's result is, bit for bit, what
  ``model(that batch, reset=True)`` returns.

A cap on the count (``max_lane_events = N >= 1``): after the time rule a lane keeps its LAST ``N`` events in arrival order
when it has more -- the newest stay, equal timestamps are cut by arrival order -- and ``dropped[b]`` (int64, cumulative,
zero after construction and after ``reset()``) grows at every step by the number the count rule removed beyond the time
rule, ``max(0, survivors + new events after the time cut - N)``.  ``t_ref``, ``t_rel``, the clock, the status bits, the lane
order and the frames are as above.  Both rules keep a suffix of the lane, so the capped window is "the time rule applied to
everything ever pushed to the lane, then the last ``N``": the same event sequence in any chunking, with the same final
``t_now``, ends in the same window.  The stream's capacity is then the constant ``B * N``: nothing grows after the first
step, a push may be larger than the capacity, and a burst costs its own lane's oldest events only.  ``window_us=None`` --
allowed only with a cap -- means ``window_us = time_window``, a pure count window.  N-Caltech101's samples are such
windows ("the last ``num_events`` events", newest at ``time_window - 1``, ``data/ncaltech101_data.py``): feed a recording to
a stream with ``window_us=None, max_lane_events=num_events`` and give the last step ``t_now = t_last + 1``; the staged
window is then ``NCaltech101.preprocess`` + ``format_data`` of the last ``num_events`` events, because
``t - (t_last - time_window + 1) = time_window - ((t_last + 1) - t)``.  With ``downsample=`` the cap counts the survivors,
the model's events.

Raw sensor events (``downsample=f`` or ``(fx, fy)``): the models read ``events_2x`` streams, the sensor's events through
the integrate-and-fire loop of ``scripts/downsample_events.py:91-124`` and cut to the model's rows
(``DSEC.preprocess_events``).  A push then carries sensor pixels of a ``sensor_size = (W_in, H_in)`` sensor (default
``(fx * W, fy * H)``), and in front of everything above:

* the cell grid is ``(W_in // fx, H_in // fy)`` and covers the model's ``(W, H)``; every lane owns an fp32 change map over
  it, zero after construction and after ``reset()``, carried from push to push;
* a lane's raw events go through their cells in arrival order: the cell adds ``p * 1.0 / (fx * fy)`` as
  ``scripts/downsample_events.py:118`` has it -- the float64 quotient, added to the fp32 cell in float64 and rounded into
  it; the increment is never rounded to fp32, which at an area ``fx * fy`` that is no power of two would keep other events
  -- with ``p`` in {-1, 0, +1}; when ``|cell| >= 1`` the event survives at ``(x // fx, y // fy)`` and ``p`` is subtracted;
* a survivor with ``x >= W`` or ``y >= H`` is dropped (the dataset's row cut), and so is an event right of / below the last
  whole cell; a raw event outside ``[0, W_in) x [0, H_in)`` is malformed (status bit of value 16);
* what is left is pushed as above, but the clock is the sensor's: the order checks run on the raw arrays, and the lane's
  newest event -- ``t_last``, and ``t_ref`` without ``t_now`` -- is its newest RAW event.

Sensor noise (``denoise_us=D`` and / or ``refractory_us=R``, each ``None`` = off or a positive int; with both ``None``
nothing changes anywhere): a background-activity filter and a refractory filter on what a push carries, before anything
else -- sensor pixels of the ``sensor_size`` sensor with ``downsample=``, the model's ``W x H`` pixels without it (the sensor
is then ``(W, H)``).  Every lane owns a stamp map ``last_t``, int64 ``[H_in, W_in]``, "never" after construction and after
``reset()``, carried from push to push.  A lane's events are taken in arrival order; for an event ``(x, y, t)`` inside the
sensor:

* supported: with ``denoise_us = D`` the event is supported if some pixel of its 8-neighbourhood has a stamp
  ``s != never`` with ``t - s <= D`` -- the centre pixel is excluded, neighbours outside the sensor do not exist, nothing
  wraps into the next row or the next lane; with ``denoise_us=None`` every event is supported;
* refractory: with ``refractory_us = R`` the event is refractory if its own pixel has a stamp ``s != never`` with
  ``t - s < R``; with ``refractory_us=None`` no event is refractory;
* kept: iff supported and not refractory;
* stamp: then ``last_t[y, x] = t``, whether the event was kept or not.

Every event stamps, so a decision depends on the timestamps of earlier events only, never on earlier decisions: the filter
is parallel (``dagr_stream_denoise``: one thread per event), and the same sequence in any chunking leaves the same
survivors and the same map.  A hot pixel with a period below ``R`` passes once and then stays silent.  "Earlier" means
arrival order: of two events with one timestamp the second sees the first (``t - s = 0``: supported, and refractory).  A raw
event outside the sensor is dropped, does not stamp and is malformed (status bit of value 16).  The survivors keep the order
of the push and go on to the integrator of ``downsample=``, or straight to the window.  The clock stays the sensor's: the
order checks run on the unfiltered push, and the lane's newest event -- ``t_last``, and ``t_ref`` without ``t_now`` -- is
its newest UNFILTERED event.  ``max_lane_events`` counts what reaches the window.  ``filtered[b]`` (int64, cumulative, zero
after construction and after ``reset()``) counts the events inside the sensor that the filter removed.

Anti-flicker and trail filters (``flicker=`` and / or ``trail_us=``; with both ``None`` nothing changes anywhere): two
per-pixel state machines on what a push carries, in front of the noise filter -- flicker events are dense and spatially
coherent, so they would otherwise count as support for the noise beside them.  The order of a step is decode, flicker /
trail, noise filter, ``downsample=``, window.  Mains- and PWM-driven lights make their pixels emit ON / OFF bursts at 100 /
120 Hz and above; an edge crossing a pixel fires a burst of same-polarity events of which the first carries the
information.  The rule below is THIS PROJECT'S statement of these two well-known filters: it is not a vendor's algorithm and
agreement with any vendor's filter is not claimed; no real camera data was at hand, the tests and measurements use
synthetic flicker; the defaults are conventions, not measured optima.  ``flicker_definition`` states the rule once in
numpy and ``dagr_stream_flicker`` repeats it.

``flicker`` is ``None``, ``True`` (the defaults) or a dict of ints ``min_hz``, ``max_hz``, ``start``, ``stop``, ``max_count``
(defaults 50, 500, 4, 1, 7) with ``1 <= min_hz <= max_hz <= 1000000`` and ``0 <= stop < start <= max_count <= 255``;
``min_period = -(-1000000 // max_hz)`` and ``max_period = 1000000 // min_hz`` in integer microseconds.  ``trail_us`` is
``None`` or a positive int.  Every lane owns, over ``[H_in, W_in]`` and carried from push to push: ``t_edge`` int64
(initially never), ``last_p`` int8 (0), ``count`` int32 (0), ``blocking`` bool (False), ``t_pass`` int64 (never), ``p_pass``
int8 (0); every field is at its initial value after construction and after ``reset()``.  A lane's events are taken in
arrival order; two events with one timestamp are two events, and the second sees the first.  An event outside
``[0, W_in) x [0, H_in)`` or with a lane outside ``[0, B)`` is skipped: outcome -1, no state touched, not counted (the
lane-less rows the decoder leaves behind its count fall under this); outside the sensor on a valid lane it raises the
status bit of value 16.  For every other event ``(t, p)``, with ``s = +1 if p > 0 else -1``:

Flicker stage (``flicker`` on):

1. stale: if ``t_edge != never`` and ``t - t_edge > max_period``, ``count = 0``;
2. edge: the event is an edge iff ``s > 0 and last_p < 0``.  On an edge with ``t_edge != never`` and ``d = t - t_edge``:
   ``count = min(count + 1, max_count)`` if ``min_period <= d <= max_period``, ``count = max(count - 1, 0)`` if
   ``d < min_period`` (``d > max_period`` was step 1).  On every edge ``t_edge = t``;
3. hysteresis: if ``count >= start``, ``blocking = True``; else if ``count <= stop``, ``blocking = False``;
4. ``last_p = s``;
5. the event passes iff ``not blocking``; otherwise its outcome is 1 and it does not reach the trail stage.

Trail stage (``trail_us`` on), for the events that passed the flicker stage, or for all when that stage is off:

1. ``trail = (p_pass == s) and (t - t_pass < trail_us)`` -- the timestamp of a never state is not subtracted;
2. ``t_pass = t`` and ``p_pass = s``, whether or not the event trailed: a continuous burst stays suppressed;
3. if ``trail``, the outcome is 2.

Anything left has outcome 0 and is kept.  All arithmetic is int64; there are no floats anywhere.  The same event sequence
in any chunking into pushes leaves the same outcomes and the same state.  The survivors keep the order of the push.  The
clock stays the sensor's, as with the noise filter: order checks, ``t_last`` and ``t_ref`` use the unfiltered (or decoded)
push.  ``suppressed()`` returns ``(flicker[B], trail[B])``, int64, cumulative, zero after construction and ``reset()``.

Frames (``--use_image`` models): every lane has a frame in force, the last one a step gave it -- as the model's image
(``image=``, fp32 [B, 3, H, W]) or as a raw sensor frame (``frame=``, uint8 [H_f, W_f, 3], which ``dagr_stream_frame``
prepares on the device; ``frame_definition`` below states what that is).  A step's result is what ``model(..., reset=True)``
returns on the window with the frames in force, whether the step ran the image branch or sampled the maps it held.

Track ids (``track=``: ``None`` is off, ``True`` takes the defaults, a dict sets ``iou`` (fp32 in (0, 1], default 0.3),
``max_age_us`` (int >= 0, default 20000), ``min_score`` (float, default 0.0) and ``max_tracks`` (1 ..
``DAGR_TRACK_MAX_TRACKS = 256``, default 64)): a step's detections are associated with the lane's tracks of the step
before, on the device, behind everything above and without changing any of it.  ``TrackDefinition`` below states it once in
numpy.  Every lane owns ``max_tracks`` slots, each free or holding a track -- ``box`` fp32[4] (x1, y1, x2, y2), ``label``
int32, ``id`` int64, ``t_last`` int64, ``hits`` int32 --, ``next_id`` int64, which starts at 1 (id 0 means "no track"), and
``untracked`` int64, cumulative; after construction and after ``reset()`` every slot is free, ``next_id = 1`` and
``untracked = 0``.  One step of lane ``b`` takes the rows ``det[b, :n_keep[b]]`` in the order ``dagr_postprocess`` leaves
them, by descending score, and the lane's ``t_ref[b]``:

1. a lane without a reference instant yet (``t_ref`` is "never"): every row gets id 0 and hits 0, nothing else happens;
2. retire: a track with ``t_ref - t_last > max_age_us`` is freed; an age equal to ``max_age_us`` stays;
3. eligible rows have ``score >= min_score`` (a NaN score is not eligible); the first ``DAGR_TRACK_MAX_DETS = 256`` eligible
   rows in row order take part, every further eligible row gets id 0 and adds 1 to ``untracked``, a row that is not eligible
   gets id 0 and is not counted;
4. match: the participating rows in row order, greedily -- among the live tracks with the row's label that no earlier row
   of this step has matched, the one with the largest IoU, the LOWEST id on a tie; if that IoU is ``>= iou`` the track takes
   the row's box, ``t_last = t_ref``, ``hits += 1``, and the row's id and hits are the track's.  A NaN IoU never matches;
5. spawn: when every row has been through 4, the participating rows that did not match take, in row order, the free slots
   in ascending slot order (slots freed in 2 count), each with ``id = next_id++`` and ``hits = 1``; without a free slot the
   row gets id 0 and adds 1 to ``untracked``.

The IoU is fp32, operation by operation: ``iw = min(ax2, bx2) - max(ax1, bx1)``, ``ih = min(ay2, by2) - max(ay1, by1)``
(``numpy.minimum`` / ``maximum``), ``inter = iw * ih if iw > 0 and ih > 0 else 0``,
``union = ((ax2 - ax1) * (ay2 - ay1) + (bx2 - bx1) * (by2 - by1)) - inter``, ``iou = inter / union`` -- the device repeats
exactly these without contraction, with a correctly rounded division.  Lanes are independent; there is no matching across
labels, and the motion model is opt-in:

A constant-velocity motion model (``motion=`` of a tracking stream: ``None`` is off, ``True`` takes the defaults, a dict
sets ``alpha``, the position gain, fp32 in (0, 1], default 1.0, and ``beta``, the velocity gain, fp32 in [0, 1], default
0.25 -- conventions of an alpha-beta filter, not measured optima).  It needs ``track=`` and ``max_age_us <= 2**24 - 1``, so
that a live track's age is exact in fp32.  Every slot additionally holds ``vel`` fp32[4], pixels per microsecond per corner
(x1, y1, x2, y2), zero in a free and in a freshly spawned slot.  ``TrackDefinition(batch_size, track, motion=...)`` states
it in numpy and ``dagr_stream_track_cv`` repeats it bit for bit, in place of ``dagr_stream_track``.  Steps 1, 2, 3 and 5
stay (a retired slot's ``vel`` is zeroed); added or replaced:

* predict, after the retirement and before any row: for every live track ``dt = fp32(t_ref - t_last)``, the int64
  difference converted as ``numpy.int64.astype(float32)`` does it -- exact inside the age bound, to the nearest even
  outside it, which takes a clock that went backwards (status bit 2) -- and ``pred[k] = box[k] + vel[k] * dt`` for the four
  corners: one fp32 multiply, then one fp32 add, no contraction.  Predictions depend on the state from before the step
  only; they are computed once per slot;
* match (replaces 4): step 4 with ``iou(row, pred)``; label rule, taken rule, largest IoU, lowest id, ``>= iou`` and NaN
  handling unchanged.  On a match, with ``z`` the row's box and ``r[k] = z[k] - pred[k]``: if ``dt > 0``,
  ``q[k] = r[k] / dt`` and ``vel[k] = q[k]`` when the track's ``hits`` was 1 (its first continuation), else
  ``vel[k] = vel[k] + beta * q[k]``; if ``dt <= 0`` ``vel`` stays.  ``box = z`` when ``alpha == 1``, else
  ``box[k] = pred[k] + alpha * r[k]``.  ``t_last = t_ref``, ``hits += 1``.  The row's outputs are the track's id and hits,
  ``track_box = box`` and ``track_vel = vel``, both after the update;
* spawn (5): the new track's ``vel`` is 0; the row's ``track_box`` is its own box and its ``track_vel`` 0 -- as for every
  row that ends with id 0 (not eligible, past ``DAGR_TRACK_MAX_DETS``, no free slot);
* coast, last: the live tracks that no row matched in this step and that were not spawned in it, in ascending slot order:
  entry ``j`` of lane ``b`` is ``coast_id[b, j]``, ``coast_box[b, j] = pred``, ``coast_label[b, j]`` and
  ``coast_age_us[b, j] = t_ref - t_last`` (int64); ``n_coast[b]`` counts them, entries at and behind it are left as they
  are.  Coasting changes no state.

A lane whose ``t_ref`` is "never" behaves as in 1; in addition ``n_coast = 0``, ``track_box`` is the row's box and
``track_vel`` 0.  So a track that moves steadily survives a gap of some steps: the returning box is compared with where the
track is predicted to be, not with where it was last seen, and in between the consumer reads the prediction from the
coast list without a host-side extrapolation.

A second association round for low-score rows (``rescue=`` of a tracking stream, with or without ``motion=``: ``None`` is
off, ``True`` takes the defaults, a dict sets ``low_score``, fp32, default 0.1, and ``iou``, fp32 in (0, 1] or ``None`` for
the tracker's own ``iou``, default ``None``).  It needs ``track=`` and ``low_score < min_score`` as fp32, so ``track``'s
``min_score`` has to be raised above its default 0.0; 0.1, and the 0.5 ``min_score`` commonly paired with it, are
ByteTrack's conventions, not measured optima.  A detector's score dips for a few steps; with one hard cut the track ages
out or comes back under a new id.  With ``rescue`` the rows under the cut may CONTINUE a track, and never start one.
``TrackDefinition(batch_size, track, motion, rescue=...)`` states it in numpy; ``dagr_stream_track_rescue`` /
``dagr_stream_track_cv_rescue`` repeat it bit for bit on the state of ``dagr_stream_track`` / ``dagr_stream_track_cv``.
The order of a step is: 1 (never), 2 (retire), predict, 4 (round one), round two, 5 (spawn), coast.  1, 2, 3, 4, 5 and the
motion model's predict, filter and coast are what they are above, over the rows of 3 (the HIGH rows); added:

* low rows have ``score >= low_score and not score >= min_score``: a NaN score is in neither band, ``score == low_score``
  is low, ``score == min_score`` is high.  The first ``DAGR_TRACK_MAX_DETS`` low rows in row order take part.  Every other
  low row, and every low row that does not match, gets what a row that is not eligible gets: id 0, hits 0, with motion its
  own box and no velocity, and it is NOT counted in ``untracked``;
* round two, when every high row has been through 4 and before any spawn: the participating low rows in row order,
  greedily, by the rule of 4 -- among the live tracks with the row's label that no row of this step, of either round, has
  matched, the one with the largest IoU (against ``box``; against ``pred`` with motion), the lowest id on a tie; a match if
  that IoU is ``>=`` rescue's ``iou``, a NaN IoU never matches.  A match does exactly what a match of 4 does (box,
  ``t_last``, ``hits += 1``, the row's outputs, with motion the same velocity and ``alpha`` filter; the track does not
  coast), and ``rescued[b] += 1``;
* spawn (5) takes the unmatched HIGH rows only: a low row never matches a track spawned in its own step and never
  occupies a slot.  Where a row stands in ``det`` does not decide its round: a low row in front of a high row waits.

``rescued`` is int64 ``[B]``, cumulative, zero after construction and after ``reset()``.  Unlike ByteTrack, round two
considers every live unmatched track, not only those seen in the step before.  Without ``rescue`` nothing of this exists.

An optimal assignment in the match (``assign=`` of a tracking stream, with or without ``motion=`` and ``rescue=``: ``None``
and ``"greedy"`` are the rules above, ``"optimal"`` is this paragraph; anything else is refused.  It needs ``track=``).
Greedy matching in row order goes wrong in a crowd: box 1 overlaps tracks A (0.6) and B (0.7), box 2 overlaps B only
(0.5); greedy gives B to box 1, box 2 spawns a new id and A is lost, where a one-to-one assignment keeps both.
``TrackDefinition(batch_size, track, motion, rescue, assign="optimal")`` states it in numpy and
``dagr_stream_track_optimal`` repeats it bit for bit on the state of ``dagr_stream_track`` / ``dagr_stream_track_cv``.  It
replaces only the MATCH of a round; never, retire, eligibility, the ``DAGR_TRACK_MAX_DETS`` cut, predict, filter, the low
rows, the spawn order, coast and ``rescued`` stay.  For a round -- round one: the participating high rows at the tracker's
``iou``; with ``rescue=`` round two: the participating low rows at rescue's ``iou``:

* ``w`` is int32 ``[rows of the round in row order, max_tracks slots in slot order]``.  ``w[r, s] = (1 << 29) + q`` if slot
  ``s`` is live (after the retirement), no earlier round of this step took it, its label equals the row's, and
  ``v = iou(row, box[s])`` (with ``motion=``: ``iou(row, pred[s])``) satisfies ``v >= `` the round's threshold -- a NaN never
  does; ``q = (int32)(v * 1048576.0f)``, an fp32 multiply and a truncating conversion,
  ``(v * np.float32(1048576)).astype(np.int32)``: the IoU is quantised to 2**-20.  Every other entry is 0;
* the pairing is ``assign_max_weight_definition(w)``'s ``row_col`` (below), and the device's is that pairing entry for
  entry.  ``256 * 2**20 < 2**29``, so the pairing has the most matches possible and, among those, the largest sum of
  quantised IoU; every weight stays below ``2**31``;
* every pair then does exactly what a match does above (box or filter, ``t_last``, ``hits += 1``, the row's outputs, in
  round two ``rescued``).  Pairs do not interact, so applying them in any order gives the same state.  Round one's
  unpaired rows spawn in row order; round two's get no id.

Most-matches-first is this project's choice, not SORT's rule, which solves on all pairs and then drops the pairs under the
threshold.  Which of several optimal pairings is taken decides track ids; it is the definition's walk -- the lowest column
on a tie -- and nothing else.  Without ``assign`` nothing of this exists.

Scoring the tracks against labelled boxes (``score=`` of a tracking stream: ``None`` is off, ``True`` takes the defaults, a
dict sets ``iou``, fp32 in (0, 1], default 0.5, ``max_objects``, 1 .. ``DAGR_SCORE_MAX_OBJECTS = 1024``, default 256, and
``boxes``, ``"det"`` (default: a hypothesis is the detection's box) or ``"track"`` (the motion model's ``track_box``; needs
``motion=``).  It needs ``track=``).  ``ScoreDefinition`` below states it once in numpy and ``dagr_stream_score`` repeats it
integer for integer, one launch behind the tracker's on the step's device arrays (``EventStream.score_step``).  It is THIS
PROJECT'S statement of the CLEAR-MOT counts (Bernardin & Stiefelhagen, "Evaluating multiple object tracking performance:
the CLEAR MOT metrics"): misses, false positives, identity switches, MOTA and MOTP, with the paper's continuity rule.  It
departs from the paper in the matcher: the assignment is greedy in ground-truth row order inside a label -- as the
tracker's own matcher and the COCO matcher of this project are -- not a minimum-cost assignment, the overlap is an IoU
and not a distance, and a label mismatch never matches.  Agreement with py-motmetrics or any other MOT tool is not
claimed.  IDF1 and HOTA need a global assignment over the whole sequence: IDF1 is ``identity=`` below, HOTA is ``hota=`` behind it.

Every lane owns an object table of ``max_objects`` slots in order of first appearance and ``n_objects``; a slot holds
``id`` int64 (the ground-truth identity, > 0), ``last_hyp`` int64 (the track id of its last match ever, 0: none),
``prev_hyp`` int64 (the track id of its match at its last scored step, 0: a miss), ``seen_step`` int64 (-1: never) and
``present``, ``tracked``, ``switches``, ``frags`` int64; and the int64 counters ``steps``, ``gt``, ``hyp``, ``match``,
``miss``, ``false_pos``, ``switch``, ``frag``, ``kept``, ``iou_q``, ``unscored_gt``, ``unscored_hyp``, cumulative, zero after
construction and after ``reset()``.  One scored step of lane ``b`` takes the step's ``det[b]``, ``n_keep[b]``,
``track_id[b]`` (and ``track_box[b]`` with ``boxes="track"``) and the ground truth ``gt_box`` fp32 ``[B, G, 4]`` (x1, y1, x2,
y2), ``gt_label`` int32 ``[B, G]``, ``gt_id`` int64 ``[B, G]``, ``n_gt`` int32 ``[B]``, ``G <= DAGR_SCORE_MAX_GT = 256``.
``n_gt[b] < 0`` means that the lane has no labels at this instant: it is skipped, and not one byte of its state changes;
``n_gt[b]`` above ``G`` is clamped.

1. hypotheses: the rows ``i < clamp(n_keep[b], 0, A)`` with ``track_id != 0``, in row order.  A row without an id is not
   tracker output: it is neither a match nor a false positive.  The first ``DAGR_TRACK_MAX_DETS`` of them take part, each
   further one adds 1 to ``unscored_hyp``.  The label is ``(int32_t)det[..., 5]``, as the tracker has it;
2. slots: the ground-truth rows in row order.  A row is unscored if its ``gt_id <= 0``, if an earlier row of this step has
   the same ``gt_id``, or if its identity is new and the table is full: it adds 1 to ``unscored_gt``, takes part in nothing
   and its outcome is -1.  Otherwise it finds its slot, or takes slot ``n_objects++``;
3. keep (CLEAR-MOT's continuity rule): the scored rows in row order whose object has ``seen_step == steps - 1`` and
   ``prev_hyp != 0``.  The FIRST hypothesis row with that id is taken; the object keeps it if that row is still free, has
   the row's label and ``iou(gt, hyp) >= iou``, and ``kept += 1``;
4. match: the remaining scored rows in row order, greedily: among the free hypotheses of the row's label the one with the
   largest IoU ``>= iou``, the LOWEST row on a tie; a NaN IoU matches nothing.  The IoU is the tracker's, ``iou(gt, hyp)``
   operation for operation in fp32 without contraction;
5. count, per scored row: ``gt += 1``, ``present += 1``, ``seen_step = steps``.  Matched to track ``h``: ``match += 1``,
   ``iou_q += (int64) rint(iou * 2**20)`` (exact and order-free: nothing is accumulated in floating point); a switch is
   counted iff ``last_hyp != 0 and last_hyp != h``, a fragmentation iff ``tracked > 0 and prev_hyp == 0``; then
   ``tracked += 1`` and ``last_hyp = prev_hyp = h``.  Unmatched: ``miss += 1``, ``prev_hyp = 0``.  An object absent from the
   step keeps its slot untouched.  Then ``hyp +=`` the participating hypotheses, ``false_pos +=`` those left free, and
   ``steps += 1``.

Per ground-truth row the step leaves ``gt_match`` int64 ``[B, G]`` (the track id, 0 for a miss, -1 for unscored) and
``gt_flags`` int32 ``[B, G]`` (bit 0 switch, bit 1 fragmentation, bit 2 kept); rows at and behind ``n_gt[b]`` and every row
of a skipped lane are left as they were.  ``score_summary`` turns counters and tables into MOTA
(``1 - (miss + false_pos + switch) / gt``), MOTP (``iou_q / 2**20 / match``, a mean IoU), precision, recall, and the
mostly tracked / mostly lost objects (``tracked / present >= 0.8`` / ``<= 0.2``).  Coasting tracks are not hypotheses, and
there are no ignore regions.  Without ``score`` nothing of this exists.

IDF1 (``identity=`` of a scoring stream: ``None`` is off, ``True`` takes the default, a dict sets ``max_tracks``,
1 .. ``DAGR_ASSIGN_MAX = 1024``, default 256.  It needs ``score=`` and takes ``iou``, ``max_objects`` and ``boxes`` from it).
IDF1 (Ristani et al., "Performance measures and a data set for multi-target, multi-camera tracking", 2016) asks for the
one-to-one pairing of object identities with track ids that maximises the frames they share.  Two definitions below state
it once in numpy and the kernels repeat them integer for integer: ``assign_max_weight_definition`` (``dagr_assign_max_weight``)
and ``IdentityDefinition`` (``dagr_stream_identity``, ``dagr_stream_identity_solve``).

The assignment: ``w`` is int ``[n, m]``, ``w >= 0``, ``n, m`` in 0 .. ``DAGR_ASSIGN_MAX``.  ``total`` is the largest sum of
``w`` over a one-to-one pairing of rows with columns and ``row_col[i]`` the column of row ``i`` in one pairing that reaches
it, -1 for a row without one; a pair of weight 0 is reported as -1.  The method is the Hungarian method by shortest
augmenting paths in integers on the cost ``-w`` with the smaller side as rows (``n > m``: the transposed matrix): potentials
``u`` (rows) and ``v`` (columns) int64, one row enters at a time, a path step marks column ``j0`` used, relaxes
``minv[j] = min(minv[j], cost[p[j0], j] - u[p[j0]] - v[j])`` over the unused columns, takes ``delta`` = the smallest ``minv``,
the LOWEST column on a tie, moves the potentials by ``delta`` and goes on from that column until it is free; then the path
is flipped.  ``total`` is unique, ``row_col`` is not: a pairing is right if it is one-to-one, lists only pairs with
``w > 0`` and sums to ``total``.  The device's pairing is nevertheless THIS walk's, entry for entry (the same relaxation, the
lowest column on a tie, the same transposition; ``tests/test_assign_pairing_gpu.py``): ``assign="optimal"`` relies on it.

The identity state: every lane owns a track table of ``max_tracks`` columns in order of first appearance (``track_id`` int64,
``track_len`` int64) and ``n_tracks``, ``obj_len`` int64 ``[max_objects]`` over the scorer's object slots, ``overlap`` int32
``[max_objects, max_tracks]`` and the int64 words ``n_objects``, ``gt_frames``, ``hyp_frames``, ``dup_hyp``, ``unlisted_hyp``,
``pairs``, ``steps``, zero after construction and after ``reset()``.  One step runs AFTER the scorer's step on the same
arrays, with the ``gt_match`` that step wrote and the scorer's id table after it; a lane with ``n_gt[b] < 0`` changes nothing:

1. hypotheses: the scorer's own rule, the rows ``i < clamp(n_keep[b], 0, A)`` with ``track_id != 0``, the first
   ``DAGR_TRACK_MAX_DETS`` in row order.  A row whose id an earlier participating row of this step carries takes no part
   and ``dup_hyp += 1``; every other row counts ``hyp_frames += 1``;
2. columns: in row order a hypothesis finds its column by id, or takes column ``n_tracks++``; with a full table it gets no
   column, ``unlisted_hyp += 1``, and its frames can only be identity false positives.  With a column ``track_len[col] += 1``;
3. rows: the ground-truth rows ``g < min(n_gt[b], G)`` with ``gt_match[b, g] != -1`` (the rows the scorer scored).  The
   object's slot is the index of ``gt_id`` in the scorer's id table (a row whose id is ``<= 0`` or not there takes no part);
   ``gt_frames += 1``, ``obj_len[slot] += 1``, ``n_objects = max(n_objects, slot + 1)``;
4. pairs: for every such row and every hypothesis with a column, when the labels are equal and ``iou(gt, hyp) >= iou`` (the
   scorer's IoU; a NaN IoU overlaps nothing): ``overlap[slot, col] += 1``, ``pairs += 1``.  This is IDF1's "all pairs that
   overlap at a step", not the scorer's one-to-one match: two objects on one hypothesis both count.  Then ``steps += 1``.

``solve()``: per lane ``idtp`` is the assignment's total on ``overlap[:n_objects, :n_tracks]``, ``idfn = gt_frames - idtp``,
``idfp = hyp_frames - idtp``, and ``obj_track[b, slot]`` is the paired track id or 0.  ``identity_summary`` gives
``idf1 = 2 idtp / (gt_frames + hyp_frames)``, ``idp = idtp / hyp_frames`` and ``idr = idtp / gt_frames`` per lane and in
total (the total sums the lanes' integers: lanes are separate sequences).  Agreement with py-motmetrics or TrackEval is
not claimed.  Without ``identity`` nothing of this exists.

HOTA (``hota=`` of an identity stream: ``None`` is off, ``True`` takes the default, a dict sets ``max_instants``,
1 .. ``DAGR_HOTA_MAX_INSTANTS = 65535``, default 1200 -- 60 s of labels at 20 Hz.  It needs ``identity=``, which needs
``score=``).  HOTA (Luiten et al., "HOTA: a higher order metric for evaluating multi-object tracking", IJCV 2021) is
``sqrt(DetA * AssA)`` over 19 localisation thresholds ``alpha = k / 20``; it needs two passes, because the matching of an
instant is weighted by an alignment score of (object, track) pairs that is known only when the whole sequence has been
seen.  A stream therefore keeps a log of its labelled instants on the device and replays it.  ``HotaDefinition`` below
states the rule once in integers and ``dagr_stream_hota`` / ``dagr_stream_hota_solve`` repeat it integer for integer.

The participants of a labelled instant of lane ``b`` (``n_gt[b] >= 0``; a skipped lane changes nothing) are what the
identity step used: the ground-truth rows that got an object slot ``s`` and the hypotheses that got a track column ``c``
(not a duplicate id, listed in the identity state's track table after its step), each in row order, boxes by the scorer's
``boxes`` option.  The similarity is ``q[g, i] = rint(fp32(iou) * 2**20)`` as an integer, the IoU ``TrackDefinition.iou``
operation for operation, 0 when the labels differ or the IoU is NaN (or outside (0, 1], which only a box with a negative
side gives).

1. a full log: with ``instants == max_instants`` the instant only adds 1 to ``dropped_instants``;
2. pass 1: ``rs[g]`` and ``cs[i]`` are the row and column sums of ``q`` in int64; for ``q > 0``
   ``pmc[s, c] += (q << 20) // (rs[g] + cs[i] - q)`` (``pmc`` int64 ``[max_objects, max_tracks]``); ``gc[s] += 1`` and
   ``tc[c] += 1`` for every participant -- HOTA's own counts, of logged instants only;
3. log: the participants' slot or column, box and label are appended; ``instants += 1``, ``rows`` and ``columns`` grow by
   the participants.  ``pmc <= 65535 * 2**20`` keeps every product below in int64.

``solve()`` is pass 2, per logged instant with the FINAL tables: ``gq[s, c] = (pmc << 20) // (((gc[s] + tc[c]) << 20) - pmc)``,
0 where ``pmc`` is 0; ``w[g, i] = (gq * q[g, i]) >> 10``, in 0 .. 2**30, compacted to the instant's rows and columns; the
pairing is ``assign_max_weight_definition``'s, entry for entry.  For ``k = 1 .. 19`` a matched pair is a TP when
``20 * q >= k << 20`` -- exact, no epsilon --: ``tp[k] += TPs``, ``fn[k] += rows - TPs``, ``fp[k] += columns - TPs``,
``loc_q[k] +=`` the TPs' ``q``, ``mc[k][s, c] += 1`` per TP.  The reduce, per lane and ``k`` in fp64 over the pairs with
``mc > 0``, one division then one multiplication a term: ``ass[k] = sum mc * (mc / (gc[s] + tc[c] - mc))``,
``re[k] = sum mc * (mc / gc[s])``, ``pr[k] = sum mc * (mc / tc[c])``.  ``hota_summary`` gives per ``k`` and as means over the
19 thresholds ``DetA = tp / max(1, tp + fn + fp)``, ``AssA = ass / max(1, tp)``, ``LocA = loc_q / (2**20 * tp)`` and
``HOTA = sqrt(DetA * AssA)``, per lane and in total.

This is THIS PROJECT'S statement of HOTA.  It departs from the usual tool: the similarities are quantised to ``2**-20``,
the alignment score is floored to ``2**-20`` and the weight to ``2**-30``, a pair of weight 0 is never matched, there is no
epsilon at the thresholds, the labels gate the similarity, and the instants behind ``max_instants`` are left out.
Agreement with TrackEval is not claimed.  Without ``hota`` nothing of this exists.

Labels at every step (``labels=``: ``None`` is off, ``True`` takes the defaults, a dict sets ``max_keyframes`` (1..65535,
default 1200), ``max_rows`` (1..``DAGR_SCORE_MAX_GT``, default 64), ``max_gap_us``, ``min_height``, ``min_diag`` (default
``None`` each); needs neither ``track`` nor ``score``).  Labels arrive far more rarely than steps -- DSEC's at 20 Hz --, so a
stream scored only where the caller holds labelled boxes is scored at one step in fifty.  The reference's inter-frame
evaluation says what the ground truth between two labelled frames is (``DSEC.__getitem__`` with ``set_num_us``:
``interpolate_tracks``, then ``filter_small_bboxes``); the stream takes the labelled keyframes once (``push_labels``) and
interpolates them to every step's own ``t_ref`` on the device (``dagr_stream_labels_at``), where the instant lives.
``LabelDefinition`` states the rule once in numpy; per lane, all arithmetic fp64, all instants int64 microseconds:

* the store is a ring of at most ``max_keyframes`` keyframes, each an instant ``t`` and ``n <= max_rows`` rows of ``xywh``
  fp64 (top-left plus size, as the DSEC tracks have it), ``label`` int32 and ``id`` int64;
* a pushed keyframe whose ``t`` is not greater than the lane's newest keyframe instant is refused (``refused``), rows beyond
  ``max_rows`` are cut (``cut_rows``), a push onto a full ring overwrites the oldest keyframe (``overwritten``);
* a step has no labels -- ``n_gt = -1``, the scorer skips the lane -- when ``t_ref`` is ``INT64_MIN``, there is no keyframe,
  or ``t_ref`` is before the oldest resident keyframe or after the newest (``outside``), or when ``max_gap_us`` is set and
  the bracketing keyframes are further apart (``gap``); every other step counts under ``labelled``, rows or none;
* inside ``[t_k, t_k+1)``, ``t_ref == t_k`` included, the rows are the identities both keyframes hold -- only ``id > 0``, an
  identity at its first row inside a keyframe -- in ascending identity (the reference's ``argsort``):
  ``r = float64(t_ref - t_k) / float64(t_k+1 - t_k)``, every one of ``x y w h`` is ``a * (1 - r) + b * r`` (two multiplies
  and one add, no contraction), the label is the earlier keyframe's;
* at the newest keyframe's own instant the rows are that keyframe's with ``id > 0``, first rows only, in ascending identity,
  as they are -- there is no extrapolation behind it;
* with ``min_height`` / ``min_diag`` a row survives iff ``sqrt(h * h + w * w) > min_diag and w > min_height and
  h > min_height`` on the fp64 values (``None``: that half is off), after the interpolation as the reference has it;
* the box is ``fp32(x), fp32(y), fp32(x + w), fp32(y + h)``, the sums in fp64.

The interpolation is linear between keyframes: it is wrong wherever the object's motion is not, and an object born or gone
between two keyframes has no row between them.  No real DSEC sequence was at hand: the rule is held to the reference's own
``interpolate_tracks`` output on the golden frames, the rest is synthetic.  A stream without ``labels`` makes exactly the
library calls it makes without the store.

The picture (``render=``: ``None`` is off, ``True`` takes the defaults, a dict sets ``event_window_us`` (``None``: every
resident event), ``alpha`` ([0, 1], default 0.5), ``linewidth`` (1..7), ``trail`` (0..64 centres, default 32), ``ids``,
``id_scale`` (1..4) and ``colors`` (uint8 ``[n, 3]`` BGR, 2 <= n <= 256)): ``render_step()`` paints one frame per lane on
the device from what the last step left there -- base, events, trails, box outlines, id plates, in this order, every pixel
on its own (``dagr_stream_render``) --, and a tracking stream with trails ends every step with ``dagr_stream_trail``, which
keeps a ring of the last centres of the track in every slot.  include/dagr_hip.h states the rule and ``RenderDefinition``
below is the same in numpy; it is not restated here.  The look is this project's own, no real camera data was at hand, and
nothing is displayed.  A stream without ``render`` makes exactly the library calls it makes without it.

Camera words (``decode="evt3"`` or ``"evt2"``): an event camera delivers words, not arrays.  A decoding stream takes the
camera's words (``step_words`` / ``step_words_device``) and decodes them on the device (``dagr_stream_decode``) in front of
everything above: decode, then the flicker / trail filters, then the noise filter, then ``downsample=``, then the window.  The two formats are stated here as
the vendor's public descriptions are recalled; no specification document, camera file or third-party decoder was at hand,
so THIS statement is the definition, ``DecodeDefinition`` below is its sequential loop and the yardstick of the kernels, and
agreement with a real camera file is not demonstrated.

Each lane owns a decoder state, carried from push to push:

- ``high``, ``low``, ``loops``: non-negative ints.
- ``y``.
- ``base_x``: uint32, additions modulo 2^32.
- ``pol``.
- ``synced``: 0 or 1.

All are 0 after construction and after ``reset()``.  A push gives every lane a run of words, possibly empty.  A lane's words
are taken in order.  Bit ranges are inclusive, with bit 0 the least significant.

EVT 3.0.  Words are little-endian uint16.  ``type = w >> 12``.

====== ============ ===============================================================================================
type   name         effect
====== ============ ===============================================================================================
0x0    ADDR_Y       ``y = w & 0x7FF``.  Bit 11 is ignored.
0x2    ADDR_X       Emits one event at ``x = w & 0x7FF`` with ``pol = (w >> 11) & 1`` (the word's own bit).
                    ``base_x`` and the state's ``pol`` are unchanged.
0x3    VECT_BASE_X  ``base_x = w & 0x7FF``, ``pol = (w >> 11) & 1``.
0x4    VECT_12      For ``i = 0..11`` ascending, where bit ``i`` of ``w`` is set, emits an event at ``x = base_x + i``
                    with the state's ``pol``.  Then ``base_x += 12``.
0x5    VECT_8       As VECT_12 with ``i = 0..7`` and ``base_x += 8``.  Bits 8..11 are ignored.
0x6    TIME_LOW     ``low = w & 0xFFF``.
0x8    TIME_HIGH    ``v = w & 0xFFF``.  If ``synced`` and ``high - v >= 2048``, then ``loops += 1``.  Then ``high = v``
                    and ``synced = 1``.  ``low`` is kept.
others              CONTINUED_4 (0x7), EXT_TRIGGER (0xA), OTHERS (0xE), CONTINUED_12 (0xF), reserved (0x1, 0x9, 0xB,
                    0xC, 0xD): no effect on the state.  ``skipped[b] += 1``.
====== ============ ===============================================================================================

Time of an emitted event: ``t = t_base[b] + (loops << 24) + (high << 12) + low``, as int64.

EVT 2.0.  Words are little-endian uint32.  ``type = w >> 28``.

========= =============== ====================================================================================
type      name            effect
========= =============== ====================================================================================
0x0 / 0x1 CD_OFF / CD_ON  Emits one event with ``low6 = (w >> 22) & 0x3F``, ``x = (w >> 11) & 0x7FF``,
                          ``y = w & 0x7FF``, ``pol = type``.
0x8       TIME_HIGH       ``v = w & 0x0FFFFFFF``.  If ``synced`` and ``high - v >= 1 << 27``, then ``loops += 1``.
                          Then ``high = v`` and ``synced = 1``.
any other                 ``skipped[b] += 1``.
========= =============== ====================================================================================

Time of an emitted event: ``t = t_base[b] + (loops << 34) + (high << 6) + low6``.

Both formats.  An emitted event goes through these checks in order:

1. If ``synced == 0``, drop it and ``unsynced[b] += 1``.  No ``TIME_HIGH`` has been seen since the reset, so the time base
   is unknown.
2. Otherwise, if not (``x < sensor_w and y < sensor_h``), drop it, ``outside[b] += 1``, and raise status bit 4 (value 16,
   "a raw event is outside the sensor").
3. Otherwise it is a decoded event ``(x, y, t, p = +1 if pol else -1, lane b)`` and ``decoded[b] += 1``.

Further rules:

- Decoded events keep word order, and bit order inside a vector word.
- Lanes are concatenated in lane order.
- The four counters are int64 ``[B]``, cumulative, and zero after construction and ``reset()``.
- A backwards ``TIME_HIGH`` jump smaller than the wrap rule makes ``t`` go backwards.  The staging's status bit 0 reports
  that, as it does for any push.
- The decoder depends on nothing but the word sequence.  Any chunking of a lane's words into pushes gives the same events,
  counters and final state.

Output buffer.  The decoded events of a push are written into buffers of ``max_out`` rows (``max_decoded=``).  If a push
decodes more than ``max_out`` events, the first ``max_out`` are kept, the state and the counters advance as if all had been
written, and status bit 6 (value 64, "decoded events exceed max_out") is raised.  ``max_decoded=None`` sizes the buffers for
the worst case of the push (12 events per EVT 3.0 word, 1 per EVT 2.0 word), so bit 6 cannot occur; a smaller value makes
the fronts behind the decoder cheaper -- they are handed all ``max_out`` rows -- and may raise it.  The decoded push is the
stream's clock: the order checks run on it, and the lane's newest event is its newest DECODED event.  The host never learns
how many events a push decoded, so its bound of the window grows by ``min(max_decoded, 12 * n_words)`` (EVT 3.0) or
``n_words`` (EVT 2.0) per step: a decoding stream that is never read back should be capped (``max_lane_events``).

Detection mAP over every step (``map=``)
----------------------------------------
The reference's inter-frame protocol is "detect between frames, evaluate against interpolated labels".  With ``map=`` the
stream keeps a log of evaluated images on the device and evaluates it where it lies.

- An image is one (lane, instant).  ``map_step()`` offers every lane's last step to the log (``dagr_stream_map_log``, one
  launch, no host wait).  A lane is logged only if it has at least one ground-truth box (``n_gt > 0``: ``evaluated_images``'
  rule); ``n_gt < 0`` counts in ``unlabelled``, ``n_gt == 0`` in ``empty``.
- A lane holds at most ``max_images`` images; later ones count in ``dropped_images`` and nothing else is written.  An image
  keeps its ``t_ref``, its ground-truth rows and its first ``min(n_keep, max_dets)`` detection rows in ``det`` order; rows
  cut count in ``cut_dets``.  Rows stay the fp32 corner rows they are.
- The images of the protocol are lane-major: all of lane 0's in log order, then lane 1's, and so on.  The order matters
  only for ties in score.
- ``map()`` builds the job list of ``utils/coco_eval.py:build_jobs`` on the device (``dagr_stream_map_plan``: count, scan,
  scatter), then runs ``dagr_coco_match`` and ``dagr_coco_accumulate`` on it.  A detection counts for the class its fp32
  label IS; labels outside ``[0, classes)`` belong to no job.  Boxes become (x, y, w, h) as ``_xywh`` does it: subtract in
  fp32, then widen.
- ``MapDefinition`` is the log's rule in numpy; its ``compute()`` hands the images to the host ``evaluate_detection``, which
  is the definition of the metric -- this project's numpy restatement of the public COCO protocol, not pycocotools.  The
  ground truth between keyframes is linear interpolation.
"""
import numpy as np

from ._lib import DEFINES, ENUMS
from .utils.synthetic import format_data_np

STATUS_BITS = ((1, "a timestamp goes backwards inside a lane (within a push or against the lane's newest event)"),
               (2, "t_now is behind the lane's newest event or behind its previous t_ref"),
               (4, "survivors plus new events exceed the stream's capacity"),
               (8, "batch is not sorted or is outside [0, batch_size)"),
               (16, "a raw event is outside the sensor (downsampling streams)"),
               (32, "a frame's lane is outside [0, batch_size)"),
               (64, "decoded events exceed max_out (a decoding stream's max_decoded)"))


def _window_and_cap(window_us, max_lane_events, time_window, batch_size, who):
    """``(window_us, max_lane_events or None)`` of a stream, checked; ``window_us=None`` is the pure count window."""
    N = max_lane_events
    if N is not None:
        if isinstance(N, bool) or not isinstance(N, (int, np.integer)) or int(N) < 1:
            raise ValueError(f"{who}: max_lane_events = {N!r} must be a positive int (or None: no cap)")
        N = int(N)
        if int(batch_size) * N >= (1 << 31) // 64:
            raise ValueError(f"{who}: batch_size * max_lane_events = {int(batch_size) * N} is outside the stream's capacity "
                             f"range (below {(1 << 31) // 64})")
    if window_us is None:
        if N is None:
            raise ValueError(f"{who}: window_us=None (a pure count window) needs max_lane_events")
        window_us = time_window
    if not 0 < int(window_us) <= int(time_window):
        raise ValueError(f"{who}: window_us = {window_us} must be in 1..time_window = {time_window} "
                         "(t_rel = time_window - age has to stay inside the model's time axis)")
    return int(window_us), N


def _factors(downsample, width, height, sensor_size, who):
    """``(fx, fy, W_in, H_in)`` of a downsampling stream over a ``width x height`` model; refusals by name."""
    f = (downsample, downsample) if np.ndim(downsample) == 0 else tuple(downsample)
    if len(f) != 2 or any(int(v) != v or int(v) < 1 for v in f):
        raise ValueError(f"{who}: downsample = {downsample!r} must be an integer factor >= 1 or a pair (fx, fy) of them")
    fx, fy = int(f[0]), int(f[1])
    w_in, h_in = (fx * width, fy * height) if sensor_size is None else (int(sensor_size[0]), int(sensor_size[1]))
    if w_in // fx < width or h_in // fy < height:
        raise ValueError(f"{who}: the cell grid {w_in // fx} x {h_in // fy} (sensor_size {w_in} x {h_in} over downsample "
                         f"{fx} x {fy}) is smaller than the model's {width} x {height}")
    if w_in > 32767 or h_in > 32767:
        raise ValueError(f"{who}: sensor_size {w_in} x {h_in} does not fit the int16 pixel coordinates")
    return fx, fy, w_in, h_in


NEVER = np.iinfo(np.int64).min          # a stamp map's "no event yet"


def _noise_options(denoise_us, refractory_us, batch_size, w_in, h_in, who):
    """``(D or None, R or None)`` of a filtering stream over a ``w_in x h_in`` sensor, checked; refusals by name."""
    out = []
    for name, v in (("denoise_us", denoise_us), ("refractory_us", refractory_us)):
        if v is not None and (isinstance(v, bool) or not isinstance(v, (int, np.integer)) or int(v) < 1):
            raise ValueError(f"{who}: {name} = {v!r} must be a positive int of microseconds (or None: off)")
        out.append(None if v is None else int(v))
    if (out[0] is not None or out[1] is not None) and int(batch_size) * int(w_in) * int(h_in) >= 1 << 31:
        raise ValueError(f"{who}: batch_size * W_in * H_in = {int(batch_size) * int(w_in) * int(h_in)} stamps are outside the "
                         f"noise filter's range (below {1 << 31})")
    return tuple(out)


def denoise_definition(last_t, x, y, t, batch, denoise_us=None, refractory_us=None):
    """The noise filter of the module docstring on one push, stated once: ``last_t`` int64 ``[B, H_in, W_in]`` is read and
    stamped in place, the result is the push's keep mask.  An event outside the sensor or with a lane outside ``[0, B)`` is
    not kept and does not stamp.  The yardstick of ``dagr_stream_denoise``; nothing on the device path calls it."""
    B, h_in, w_in = last_t.shape
    keep = np.zeros(len(t), bool)
    D, R = denoise_us, refractory_us
    for i in range(len(t)):
        xi, yi, ti, b = int(x[i]), int(y[i]), int(t[i]), int(batch[i])
        if not (0 <= xi < w_in and 0 <= yi < h_in and 0 <= b < B):
            continue
        lane = last_t[b]
        supported = D is None
        if not supported:
            near = lane[max(yi - 1, 0):yi + 2, max(xi - 1, 0):xi + 2]
            stamped = near != NEVER
            ok = stamped & (ti - np.where(stamped, near, ti) <= D)          # (int64 throughout; never is not subtracted)
            ok[min(yi, 1), min(xi, 1)] = False                              # the centre pixel
            supported = bool(ok.any())
        own = int(lane[yi, xi])
        refractory = R is not None and own != NEVER and ti - own < R
        keep[i] = supported and not refractory
        lane[yi, xi] = ti
    return keep


FLICKER_DEFAULTS = dict(min_hz=50, max_hz=500, start=4, stop=1, max_count=7)       # conventions, not measured optima
FLICKER_STATE = (("t_edge", np.int64, NEVER), ("last_p", np.int8, 0), ("count", np.int32, 0), ("blocking", np.bool_, False),
                 ("t_pass", np.int64, NEVER), ("p_pass", np.int8, 0))


def flicker_state(batch_size, w_in, h_in):
    """The initial state of ``flicker_definition``: a dict of one ``[B, H_in, W_in]`` array per field of ``FLICKER_STATE``."""
    return {name: np.full((int(batch_size), int(h_in), int(w_in)), first, dtype) for name, dtype, first in FLICKER_STATE}


def _flicker_options(flicker, trail_us, batch_size, w_in, h_in, who):
    """``(flicker dict or None, trail_us or None)`` of a stream over a ``w_in x h_in`` sensor, checked: ``flicker`` is None
    (off), True (the defaults) or a dict of ints ``min_hz``, ``max_hz``, ``start``, ``stop``, ``max_count``; ``trail_us`` is
    None (off) or a positive int.  Refusals by name."""
    opt = _options(flicker, "flicker", FLICKER_DEFAULTS, who)
    if opt is not None:
        for name, v in opt.items():
            if not _is_int(v):
                raise ValueError(f"{who}: flicker {name} = {v!r} must be an int")
        opt = {name: int(v) for name, v in opt.items()}
        if not 1 <= opt["min_hz"] <= opt["max_hz"] <= 1000000:
            raise ValueError(f"{who}: flicker min_hz = {opt['min_hz']} and max_hz = {opt['max_hz']} must satisfy "
                             "1 <= min_hz <= max_hz <= 1000000")
        if not 0 <= opt["stop"] < opt["start"] <= opt["max_count"] <= 255:
            raise ValueError(f"{who}: flicker stop = {opt['stop']}, start = {opt['start']} and max_count = "
                             f"{opt['max_count']} must satisfy 0 <= stop < start <= max_count <= 255")
    if trail_us is not None and (not _is_int(trail_us) or int(trail_us) < 1):
        raise ValueError(f"{who}: trail_us = {trail_us!r} must be a positive int of microseconds (or None: off)")
    trail_us = None if trail_us is None else int(trail_us)
    if (opt is not None or trail_us is not None) and int(batch_size) * int(w_in) * int(h_in) >= 1 << 31:
        raise ValueError(f"{who}: batch_size * W_in * H_in = {int(batch_size) * int(w_in) * int(h_in)} pixel states are "
                         f"outside the flicker / trail filter's range (below {1 << 31})")
    return opt, trail_us


def flicker_periods(opt):
    """``(min_period, max_period)`` in integer microseconds of checked flicker options: the edge periods that count."""
    return -(-1000000 // opt["max_hz"]), 1000000 // opt["min_hz"]


def flicker_definition(state, x, y, t, p, batch, flicker=None, trail_us=None):
    """The anti-flicker and trail filters of the module docstring on one push, stated once: ``state`` (``flicker_state``)
    is read and updated in place, the result is an int8 outcome per event -- 0 kept, 1 removed by the flicker stage, 2
    removed by the trail stage, -1 not an event of this sensor (outside it, or a lane outside ``[0, B)``: no state is
    touched).  The yardstick of ``dagr_stream_flicker``; nothing on the device path calls it."""
    B, h_in, w_in = state["t_edge"].shape
    opt, trail_us = _flicker_options(flicker, trail_us, B, w_in, h_in, "flicker_definition")
    if opt is not None:
        min_period, max_period = flicker_periods(opt)
    t_edge, last_p, count, blocking = state["t_edge"], state["last_p"], state["count"], state["blocking"]
    t_pass, p_pass = state["t_pass"], state["p_pass"]
    out = np.full(len(t), -1, np.int8)
    for i in range(len(t)):
        xi, yi, ti, b = int(x[i]), int(y[i]), int(t[i]), int(batch[i])
        if not (0 <= xi < w_in and 0 <= yi < h_in and 0 <= b < B):
            continue
        at = (b, yi, xi)
        s = 1 if int(p[i]) > 0 else -1
        out[i] = 0
        if opt is not None:
            edge_t = int(t_edge[at])
            if edge_t != NEVER and ti - edge_t > max_period:               # stale
                count[at] = 0
            if s > 0 and last_p[at] < 0:                                    # an OFF -> ON edge
                if edge_t != NEVER:
                    d = ti - edge_t
                    if min_period <= d <= max_period:
                        count[at] = min(int(count[at]) + 1, opt["max_count"])
                    elif d < min_period:
                        count[at] = max(int(count[at]) - 1, 0)
                t_edge[at] = ti
            if count[at] >= opt["start"]:
                blocking[at] = True
            elif count[at] <= opt["stop"]:
                blocking[at] = False
            last_p[at] = s
            if blocking[at]:
                out[i] = 1
                continue
        if trail_us is not None:
            trail = int(p_pass[at]) == s and ti - int(t_pass[at]) < trail_us    # (p_pass == s: t_pass is not never)
            t_pass[at], p_pass[at] = ti, s
            if trail:
                out[i] = 2
    return out


DAGR_TRACK_MAX_TRACKS = DEFINES["DAGR_TRACK_MAX_TRACKS"]       # include/dagr_hip.h states them; the binding reads it
DAGR_TRACK_MAX_DETS = DEFINES["DAGR_TRACK_MAX_DETS"]
TRACK_DEFAULTS = dict(iou=0.3, max_age_us=20000, min_score=0.0, max_tracks=64)
TRACK_DTYPE = [("id", "<i8"), ("x1", "<f4"), ("y1", "<f4"), ("x2", "<f4"), ("y2", "<f4"), ("label", "<i4"),
               ("t_last", "<i8"), ("hits", "<i4")]


def _is_int(v):
    return not isinstance(v, bool) and isinstance(v, (int, np.integer))


def _is_real(v):
    return not isinstance(v, bool) and isinstance(v, (int, float, np.integer, np.floating)) and v == v


def _options(value, name, defaults, who):
    """``name=`` of a stream (``track=``, ``motion=``): None stays None (off), True is ``defaults``, a dict has the defaults
    filled in; anything else, and a key that ``defaults`` does not have, is refused by name."""
    if value is None:
        return None
    if value is True:
        value = {}
    if not isinstance(value, dict):
        raise ValueError(f"{who}: {name} = {value!r} must be None (off), True (the defaults) or a dict of "
                         f"{', '.join(defaults)}")
    unknown = sorted(set(value) - set(defaults))
    if unknown:
        raise ValueError(f"{who}: {name} has no option {unknown[0]!r} (it has {', '.join(defaults)})")
    return dict(defaults, **value)


def _track_options(track, who):
    """``track=`` of a stream, checked: None (off) or the dict of ``iou``, ``max_age_us``, ``min_score`` and ``max_tracks``
    with the defaults filled in; refusals by name."""
    opt = _options(track, "track", TRACK_DEFAULTS, who)
    if opt is None:
        return None
    if not _is_real(opt["iou"]) or not 0 < np.float32(opt["iou"]) <= 1:
        raise ValueError(f"{who}: track iou = {opt['iou']!r} must be a float in (0, 1] (as fp32)")
    if not _is_int(opt["max_age_us"]) or not 0 <= int(opt["max_age_us"]) < 1 << 63:
        raise ValueError(f"{who}: track max_age_us = {opt['max_age_us']!r} must be an int of microseconds >= 0")
    if not _is_real(opt["min_score"]):
        raise ValueError(f"{who}: track min_score = {opt['min_score']!r} must be a float (not NaN)")
    if not _is_int(opt["max_tracks"]) or not 1 <= int(opt["max_tracks"]) <= DAGR_TRACK_MAX_TRACKS:
        raise ValueError(f"{who}: track max_tracks = {opt['max_tracks']!r} must be an int in 1..DAGR_TRACK_MAX_TRACKS = "
                         f"{DAGR_TRACK_MAX_TRACKS}")
    return dict(iou=float(np.float32(opt["iou"])), max_age_us=int(opt["max_age_us"]),
                min_score=float(np.float32(opt["min_score"])), max_tracks=int(opt["max_tracks"]))


MOTION_DEFAULTS = dict(alpha=1.0, beta=0.25)        # conventions (a plain alpha-beta filter), not measured optima
MOTION_MAX_AGE_US = DEFINES["DAGR_TRACK_CV_MAX_AGE_US"]        # 2**24 - 1: a live track's age is exact in fp32
TRACK_MOTION_DTYPE = TRACK_DTYPE + [("vx1", "<f4"), ("vy1", "<f4"), ("vx2", "<f4"), ("vy2", "<f4")]
COAST_DTYPE = [("id", "<i8"), ("x1", "<f4"), ("y1", "<f4"), ("x2", "<f4"), ("y2", "<f4"), ("label", "<i4"), ("age_us", "<i8")]


def _motion_options(motion, track_options, who):
    """``motion=`` of a tracking stream, checked: None (off) or the dict of ``alpha`` and ``beta`` (as fp32) with the
    defaults filled in; ``track_options`` is what ``_track_options`` returned.  Refusals by name."""
    opt = _options(motion, "motion", MOTION_DEFAULTS, who)
    if opt is None:
        return None
    if track_options is None:
        raise ValueError(f"{who}: motion= needs track= (the motion model is the tracker's)")
    if not _is_real(opt["alpha"]) or not 0 < np.float32(opt["alpha"]) <= 1:
        raise ValueError(f"{who}: motion alpha = {opt['alpha']!r} must be a float in (0, 1] (as fp32)")
    if not _is_real(opt["beta"]) or not 0 <= np.float32(opt["beta"]) <= 1:
        raise ValueError(f"{who}: motion beta = {opt['beta']!r} must be a float in [0, 1] (as fp32)")
    if track_options["max_age_us"] > MOTION_MAX_AGE_US:
        raise ValueError(f"{who}: track max_age_us = {track_options['max_age_us']} must not exceed {MOTION_MAX_AGE_US} "
                         "(2**24 - 1) with motion=: a live track's age has to be exact in fp32")
    return dict(alpha=float(np.float32(opt["alpha"])), beta=float(np.float32(opt["beta"])))


RESCUE_DEFAULTS = dict(low_score=0.1, iou=None)     # ByteTrack's conventions, not measured optima; iou None: the tracker's


def _rescue_options(rescue, track_options, who):
    """``rescue=`` of a tracking stream, checked: None (off) or the dict of ``low_score`` and ``iou`` (as fp32) with the
    defaults filled in and ``iou = None`` resolved to the tracker's own ``iou``; ``track_options`` is what
    ``_track_options`` returned.  Refusals by name."""
    opt = _options(rescue, "rescue", RESCUE_DEFAULTS, who)
    if opt is None:
        return None
    if track_options is None:
        raise ValueError(f"{who}: rescue= needs track= (the second round is the tracker's)")
    if not _is_real(opt["low_score"]):
        raise ValueError(f"{who}: rescue low_score = {opt['low_score']!r} must be a float (not NaN)")
    if opt["iou"] is not None and (not _is_real(opt["iou"]) or not 0 < np.float32(opt["iou"]) <= 1):
        raise ValueError(f"{who}: rescue iou = {opt['iou']!r} must be a float in (0, 1] (as fp32), or None: track's iou")
    low, cut = np.float32(opt["low_score"]), np.float32(track_options["min_score"])
    if not low < cut:
        raise ValueError(f"{who}: rescue low_score = {float(low)!r} must be below track min_score = {float(cut)!r} (as fp32): "
                         "no score lies in between; raise track's min_score")
    return dict(low_score=float(low), iou=float(np.float32(track_options["iou"] if opt["iou"] is None else opt["iou"])))


ASSIGN_ONE = 1 << 29            # what an admissible pair weighs before its IoU: above 256 quantised IoUs, so matches count first
ASSIGN_IOU_ONE = 1 << 20        # the IoU of a pair is quantised to 2**-20


def _assign_options(assign, track_options, who):
    """``assign=`` of a tracking stream, checked: None and ``"greedy"`` are None (the greedy match), ``"optimal"`` stays;
    ``track_options`` is what ``_track_options`` returned.  Refusals by name."""
    if assign is None:
        return None
    if not isinstance(assign, str) or assign not in ("greedy", "optimal"):
        raise ValueError(f"{who}: assign = {assign!r} must be None or 'greedy' (the greedy match) or 'optimal' (an optimal "
                         "assignment per round)")
    if track_options is None:
        raise ValueError(f"{who}: assign= needs track= (the assignment is the tracker's match)")
    return None if assign == "greedy" else assign


class TrackDefinition:
    """The tracker of the module docstring in numpy: ``step(det, n_keep, t_ref)`` is one step of every lane and returns
    ``(track_id int64 [B, A], track_hits int32 [B, A])`` with the rows at and behind ``n_keep[b]`` zero.  The state is the
    slots' arrays ``id`` (0: free), ``t_last``, ``box``, ``label``, ``hits`` over ``[B, max_tracks]``, ``next_id`` and
    ``untracked`` over ``[B]``.  ``events`` counts what has happened so far (matches, spawns, retirements, slots taken
    again, untracked rows) so that a test can tell a run that exercises the rules from one that does not.  The yardstick of
    ``dagr_stream_track``; nothing on the device path calls it.

    With ``motion`` (``True`` or a dict of ``alpha``, ``beta``) it is the constant-velocity tracker of the module docstring,
    the yardstick of ``dagr_stream_track_cv``: the slots also hold ``vel`` fp32 ``[B, max_tracks, 4]``, and a step leaves
    ``track_box`` / ``track_vel`` fp32 ``[B, A, 4]`` (zero at and behind ``n_keep[b]``), ``n_coast`` int32 ``[B]`` and
    ``coast_id``, ``coast_box``, ``coast_label``, ``coast_age_us`` over ``[B, max_tracks]``, whose entries at and behind
    ``n_coast[b]`` are left as they were.  ``events`` then also counts ``coasted`` track-steps and ``motion_only``, the
    matches for which no free track of the row's label had an IoU ``>= iou`` with its UNPREDICTED box -- rows the plain
    rule would have spawned.  Without ``motion`` nothing of this exists and every result is what it was.

    With ``rescue`` (``True`` or a dict of ``low_score``, ``iou``) the step has the second association round of the module
    docstring, with or without ``motion``: the yardstick of ``dagr_stream_track_rescue`` / ``dagr_stream_track_cv_rescue``.
    ``rescued`` int64 ``[B]`` counts the matches of round two, and so does ``events["rescued"]``.  Without ``rescue``
    neither exists and every result is what it was.

    With ``assign="optimal"`` the match of every round is the optimal assignment of the module docstring, with ``motion``
    and ``rescue`` composing as they do without it: the yardstick of ``dagr_stream_track_optimal``.  ``events`` then also
    counts ``conflicts``, the rounds (of one lane and one step) in which some row or some track had two or more admissible
    partners, and ``reassigned``, the rounds whose pairing differs from what the greedy rule gives on the same state; and
    ``rounds`` lists, for the LAST step, ``dict(lane, second, rows, w, row_col, greedy)`` per round that had rows -- the
    weights, the pairing and the greedy rule's pairing, slots by row, -1 for none.  ``motion_only`` then asks whether an
    unpredicted box of a track that was untaken when the round began reaches the round's threshold.  Without ``assign``
    (``None`` or ``"greedy"``) nothing of this exists and every result is what it was."""

    def __init__(self, batch_size, track=True, motion=None, rescue=None, assign=None):
        self.B = int(batch_size)
        self.options = _track_options(track, "TrackDefinition")
        self.motion = _motion_options(motion, self.options, "TrackDefinition")
        self.rescue = _rescue_options(rescue, self.options, "TrackDefinition")
        self.assign = _assign_options(assign, self.options, "TrackDefinition")
        if self.options is None:
            raise ValueError("TrackDefinition: track = None is a stream that does not track")
        self.reset()

    def reset(self):
        B, M = self.B, self.options["max_tracks"]
        self.id, self.t_last = np.zeros((B, M), np.int64), np.zeros((B, M), np.int64)
        self.box = np.zeros((B, M, 4), np.float32)
        self.label, self.hits = np.zeros((B, M), np.int32), np.zeros((B, M), np.int32)
        self.next_id, self.untracked = np.ones(B, np.int64), np.zeros(B, np.int64)
        self._used = np.zeros((B, M), bool)
        self.events = dict(matched=0, spawned=0, retired=0, reused=0, untracked=0)
        if self.motion is not None:
            self.vel = np.zeros((B, M, 4), np.float32)
            self.track_box = self.track_vel = None
            self.n_coast = np.zeros(B, np.int32)
            self.coast_id, self.coast_age_us = np.zeros((B, M), np.int64), np.zeros((B, M), np.int64)
            self.coast_box, self.coast_label = np.zeros((B, M, 4), np.float32), np.zeros((B, M), np.int32)
            self.events.update(coasted=0, motion_only=0)
        if self.rescue is not None:
            self.rescued = np.zeros(B, np.int64)
            self.events.update(rescued=0)
        if self.assign is not None:
            self.rounds = []
            self.events.update(conflicts=0, reassigned=0)

    @staticmethod
    def iou(a, b):
        """fp32, operation by operation as ``dagr_stream_track`` repeats them; ``a`` the row, ``b`` the track."""
        f = np.float32
        a, b = [f(v) for v in a], [f(v) for v in b]
        with np.errstate(all="ignore"):
            iw = f(np.minimum(a[2], b[2]) - np.maximum(a[0], b[0]))
            ih = f(np.minimum(a[3], b[3]) - np.maximum(a[1], b[1]))
            inter = f(iw * ih) if iw > 0 and ih > 0 else f(0)
            union = f(f(f(f(a[2] - a[0]) * f(a[3] - a[1])) + f(f(b[2] - b[0]) * f(b[3] - b[1]))) - inter)
            return f(inter / union)

    def step(self, det, n_keep, t_ref):
        """One step of every lane.  With ``motion``: predict, match against the predictions, filter, spawn at rest, coast.
        With ``rescue``: the low rows go through the match behind the high rows and in front of the spawn."""
        f = np.float32
        det = np.asarray(det, np.float32)
        B, A = det.shape[:2]
        if B != self.B or det.shape[2] != 6:
            raise ValueError(f"TrackDefinition: det is fp32 [{self.B}, A, 6], got {det.shape}")
        n_keep = np.broadcast_to(np.asarray(n_keep, np.int64).reshape(-1), (B,))
        t_ref = np.broadcast_to(np.asarray(t_ref, np.int64).reshape(-1), (B,))
        o, motion, rescue = self.options, self.motion is not None, self.rescue is not None
        thr, min_score = f(o["iou"]), f(o["min_score"])
        if rescue:
            low_score, low_thr = f(self.rescue["low_score"]), f(self.rescue["iou"])
        ids, hits = np.zeros((B, A), np.int64), np.zeros((B, A), np.int32)
        if motion:
            alpha, beta = f(self.motion["alpha"]), f(self.motion["beta"])
            self.track_box, self.track_vel = np.zeros((B, A, 4), np.float32), np.zeros((B, A, 4), np.float32)
        if self.assign is not None:
            self.rounds = []
        for b in range(B):
            n, now = min(max(int(n_keep[b]), 0), A), int(t_ref[b])
            if motion:
                self.track_box[b, :n] = det[b, :n, :4]             # a row without a track: its own box, no velocity
            if now == NEVER:
                if motion:
                    self.n_coast[b] = 0
                continue
            for s in np.flatnonzero(self.id[b]):                   # retire
                if now - int(self.t_last[b, s]) > o["max_age_us"]:
                    self.id[b, s] = 0
                    if motion:
                        self.vel[b, s] = 0
                    self.events["retired"] += 1
            live = [int(s) for s in np.flatnonzero(self.id[b])]
            # what a row is compared with: the slot's box, or where the motion model predicts it.  Either is from before
            # the step: a matched slot is taken and never compared again, and the spawns come behind the rows
            against = self.box[b]
            if motion:
                dt, pred = {}, {}
                with np.errstate(all="ignore"):
                    for s in live:                                 # predict, once
                        dt[s] = (np.int64(now) - self.t_last[b, s]).astype(f)
                        pred[s] = np.array([f(self.box[b, s, k] + f(self.vel[b, s, k] * dt[s])) for k in range(4)], f)
                against = pred
            eligible = [i for i in range(n) if det[b, i, 4] >= min_score]         # (a NaN score compares false)
            lost = max(0, len(eligible) - DAGR_TRACK_MAX_DETS)
            unmatched, taken = [], set()
            rows = [(i, thr, False) for i in eligible[:DAGR_TRACK_MAX_DETS]]
            if rescue:                                             # round two: the low rows, behind every high row
                low = [i for i in range(n) if det[b, i, 4] >= low_score and not det[b, i, 4] >= min_score]
                rows += [(i, low_thr, True) for i in low[:DAGR_TRACK_MAX_DETS]]
            def matches(i, label, s, bar, second, gone):            # what a match does, in either round, under either rule
                z = det[b, i, :4]
                if motion and not any(self.iou(z, self.box[b, c]) >= bar for c in live
                                      if c not in gone and int(self.label[b, c]) == label):
                    self.events["motion_only"] += 1                # (the plain rule would have spawned this row)
                taken.add(s)
                if motion:                                         # filter: the row pulls box and vel off the prediction
                    with np.errstate(all="ignore"):
                        r = np.array([f(z[k] - pred[s][k]) for k in range(4)], f)
                        if dt[s] > 0:
                            q = np.array([f(r[k] / dt[s]) for k in range(4)], f)
                            self.vel[b, s] = q if self.hits[b, s] == 1 else \
                                np.array([f(self.vel[b, s, k] + f(beta * q[k])) for k in range(4)], f)
                        self.box[b, s] = z if alpha == 1 else np.array([f(pred[s][k] + f(alpha * r[k])) for k in range(4)], f)
                else:
                    self.box[b, s] = z
                self.t_last[b, s] = now
                self.hits[b, s] += 1
                ids[b, i], hits[b, i] = self.id[b, s], self.hits[b, s]
                if motion:
                    self.track_box[b, i], self.track_vel[b, i] = self.box[b, s], self.vel[b, s]
                self.events["matched"] += 1
                if second:
                    self.rescued[b] += 1
                    self.events["rescued"] += 1

            if self.assign is not None:                            # match: one optimal assignment per round
                for second in (False, True)[:2 if rescue else 1]:
                    members = [i for i, _, sec in rows if sec == second]
                    if not members:
                        continue
                    bar = low_thr if second else thr
                    w, greedy = self._round_weights(b, det, members, live, taken, against, bar)
                    row_col = assign_max_weight_definition(w)[1]
                    self.events["conflicts"] += int(((w > 0).sum(0) > 1).any() or ((w > 0).sum(1) > 1).any())
                    self.events["reassigned"] += int(not np.array_equal(row_col, greedy))
                    self.rounds.append(dict(lane=b, second=second, rows=members, w=w, row_col=row_col, greedy=greedy))
                    before = set(taken)
                    for i, s in zip(members, row_col):
                        with np.errstate(all="ignore"):
                            label = int(det[b, i, 5].astype(np.int32))
                        if s >= 0:
                            matches(i, label, int(s), bar, second, before)
                        elif not second:
                            unmatched.append((i, label))
                rows = []
            for i, bar, second in rows:                            # match: the rule of both rounds
                with np.errstate(all="ignore"):
                    label = int(det[b, i, 5].astype(np.int32))
                best, best_s = None, None
                for s in live:
                    if s in taken or int(self.label[b, s]) != label:
                        continue
                    v = self.iou(det[b, i, :4], against[s])
                    if not v >= bar:                               # (a NaN IoU never matches)
                        continue
                    if best is None or v > best or (v == best and self.id[b, s] < self.id[b, best_s]):
                        best, best_s = v, s
                if best_s is None:
                    if not second:                                 # (a low row never spawns and is not counted)
                        unmatched.append((i, label))
                    continue
                matches(i, label, best_s, bar, second, taken)
            free = [int(s) for s in np.flatnonzero(self.id[b] == 0)]
            for (i, label), s in zip(unmatched, free):             # spawn (with motion: at rest)
                self.id[b, s], self.t_last[b, s], self.box[b, s] = self.next_id[b], now, det[b, i, :4]
                if motion:
                    self.vel[b, s] = 0
                self.label[b, s], self.hits[b, s] = label, 1
                ids[b, i], hits[b, i] = self.next_id[b], 1
                self.next_id[b] += 1
                self.events["spawned"] += 1
                self.events["reused"] += int(self._used[b, s])
                self._used[b, s] = True
            lost += max(0, len(unmatched) - len(free))
            self.untracked[b] += lost
            self.events["untracked"] += lost
            if motion:
                coast = [s for s in live if s not in taken]        # coast: lived before the rows, seen by none; slot order
                for j, s in enumerate(coast):
                    self.coast_id[b, j], self.coast_box[b, j], self.coast_label[b, j] = self.id[b, s], pred[s], self.label[b, s]
                    self.coast_age_us[b, j] = np.int64(now) - self.t_last[b, s]
                self.n_coast[b] = len(coast)
                self.events["coasted"] += len(coast)
        return ids, hits

    def _round_weights(self, b, det, members, live, taken, against, bar):
        """One round of ``assign="optimal"``: ``w`` int32 ``[rows of the round, max_tracks]`` as the module docstring states
        it, and, slots by row (-1: none), what the greedy rule pairs on the same state."""
        M = self.options["max_tracks"]
        w, v = np.zeros((len(members), M), np.int32), {}
        for r, i in enumerate(members):
            with np.errstate(all="ignore"):
                label = int(det[b, i, 5].astype(np.int32))
                for s in live:
                    if s in taken or int(self.label[b, s]) != label:
                        continue
                    v[r, s] = self.iou(det[b, i, :4], against[s])
                    if v[r, s] >= bar:                             # (a NaN IoU never does)
                        w[r, s] = ASSIGN_ONE + (v[r, s] * np.float32(ASSIGN_IOU_ONE)).astype(np.int32)
        greedy, gone = np.full(len(members), -1, np.int64), set()
        for r in range(len(members)):
            best = None
            for s in np.flatnonzero(w[r]):
                s = int(s)
                if s not in gone and (best is None or v[r, s] > v[r, best] or
                                      (v[r, s] == v[r, best] and self.id[b, s] < self.id[b, best])):
                    best = s
            if best is not None:
                greedy[r] = best
                gone.add(best)
        return w, greedy

    def coasting(self):
        """Per lane the last step's coasting tracks, a ``COAST_DTYPE`` array in slot order (``EventStream.coasting()``)."""
        if self.motion is None:
            raise RuntimeError("TrackDefinition: no motion model (motion=): nothing coasts")
        return [coast_from_arrays(int(self.n_coast[b]), self.coast_id[b], self.coast_box[b], self.coast_label[b],
                                  self.coast_age_us[b]) for b in range(self.B)]

    def tracks(self):
        """Per lane the live tracks as a ``TRACK_DTYPE`` array sorted by id (what ``EventStream.tracks()`` returns); with
        ``motion``, ``TRACK_MOTION_DTYPE``: the velocities appended."""
        vel = self.vel if self.motion is not None else [None] * self.B
        return [tracks_from_arrays(self.id[b], self.t_last[b], self.box[b], self.label[b], self.hits[b], vel[b])
                for b in range(self.B)]


def tracks_from_arrays(ids, t_last, box, label, hits, vel=None):
    """One lane's slots -> its live tracks, a ``TRACK_DTYPE`` array sorted by id (``TRACK_MOTION_DTYPE`` with ``vel``)."""
    live = np.flatnonzero(ids)
    live = live[np.argsort(ids[live], kind="stable")]
    out = np.zeros(len(live), TRACK_DTYPE if vel is None else TRACK_MOTION_DTYPE)
    out["id"], out["t_last"], out["label"], out["hits"] = ids[live], t_last[live], label[live], hits[live]
    for k, name in enumerate(("x1", "y1", "x2", "y2")):
        out[name] = box[live, k]
        if vel is not None:
            out["v" + name] = vel[live, k]
    return out


def coast_from_arrays(n, ids, box, label, age_us):
    """One lane's coast list -> its first ``n`` entries as a ``COAST_DTYPE`` array, in slot order."""
    out = np.zeros(n, COAST_DTYPE)
    out["id"], out["label"], out["age_us"] = ids[:n], label[:n], age_us[:n]
    for k, name in enumerate(("x1", "y1", "x2", "y2")):
        out[name] = box[:n, k]
    return out


DAGR_SCORE_MAX_OBJECTS = DEFINES["DAGR_SCORE_MAX_OBJECTS"]
DAGR_SCORE_MAX_GT = DEFINES["DAGR_SCORE_MAX_GT"]
SCORE_DEFAULTS = dict(iou=0.5, max_objects=256, boxes="det")
SCORE_COUNTERS = ("steps", "gt", "hyp", "match", "miss", "false_pos", "switch", "frag", "kept", "iou_q", "unscored_gt",
                  "unscored_hyp")
SCORE_OBJECT_FIELDS = ("id", "last_hyp", "prev_hyp", "seen_step", "present", "tracked", "switches", "frags")
SCORE_OBJECT_DTYPE = [(name, "<i8") for name in SCORE_OBJECT_FIELDS]
SCORE_SWITCH, SCORE_FRAG, SCORE_KEPT = 1, 2, 4          # the bits of gt_flags
SCORE_IOU_ONE = 1 << 20                                 # iou_q counts IoUs in units of 2**-20


def _score_options(score, track_options, motion_options, who):
    """``score=`` of a tracking stream, checked: None (off) or the dict of ``iou`` (as fp32), ``max_objects`` and ``boxes``
    with the defaults filled in; ``track_options`` / ``motion_options`` are what ``_track_options`` / ``_motion_options``
    returned.  Refusals by name."""
    opt = _options(score, "score", SCORE_DEFAULTS, who)
    if opt is None:
        return None
    if track_options is None:
        raise ValueError(f"{who}: score= needs track= (it scores the tracker's ids)")
    if not _is_real(opt["iou"]) or not 0 < np.float32(opt["iou"]) <= 1:
        raise ValueError(f"{who}: score iou = {opt['iou']!r} must be a float in (0, 1] (as fp32)")
    if not _is_int(opt["max_objects"]) or not 1 <= int(opt["max_objects"]) <= DAGR_SCORE_MAX_OBJECTS:
        raise ValueError(f"{who}: score max_objects = {opt['max_objects']!r} must be an int in 1..DAGR_SCORE_MAX_OBJECTS = "
                         f"{DAGR_SCORE_MAX_OBJECTS}")
    if opt["boxes"] not in ("det", "track"):
        raise ValueError(f"{who}: score boxes = {opt['boxes']!r} must be 'det' (the detection's box) or 'track' (the motion "
                         "model's track_box)")
    if opt["boxes"] == "track" and motion_options is None:
        raise ValueError(f"{who}: score boxes = 'track' needs motion= (track_box is the motion model's)")
    return dict(iou=float(np.float32(opt["iou"])), max_objects=int(opt["max_objects"]), boxes=opt["boxes"])


def _labelled_step(who, batch_size, boxes, det, n_keep, track_id, gt_box, gt_label, gt_id, n_gt, track_box, **tables):
    """What the labelled step's definitions (``ScoreDefinition``, ``IdentityDefinition``, ``HotaDefinition``: ``who``)
    share before their loop over the lanes; ``stream_eval.hpp`` is the same rule on the device.  The arrays coerced and
    their shapes refused by name; ``tables`` are the int64 arrays a later definition takes besides, ``name=(array, width)``
    for ``[B, width]`` and ``width = None`` for ``[B, G]``.  Returns ``(track_id, boxes, labels, gt_box, gt_label, gt_id, n,
    ng, *tables)``: ``boxes`` fp32 ``[B, A, 4]`` is ``track_box`` or the detections' as ``boxes=`` of the score options has
    it, ``labels`` int32 ``[B, A]`` the detections' classes, ``n`` int64 ``[B]`` the lane's ``n_keep`` inside ``0..A`` and
    ``ng`` its ``n_gt`` (None: ``G``) capped at ``G`` -- negative: the lane has no labels at this instant."""
    det, track_id = np.asarray(det, np.float32), np.asarray(track_id, np.int64)
    B, A = det.shape[:2]
    gt_box, gt_label, gt_id = np.asarray(gt_box, np.float32), np.asarray(gt_label, np.int32), np.asarray(gt_id, np.int64)
    G = gt_box.shape[1] if gt_box.ndim == 3 else -1
    names = list(tables)
    widths = [tables[name][1] for name in names]
    tables = [np.asarray(tables[name][0], np.int64) for name in names]
    if B != batch_size or det.shape[2:] != (6,) or track_id.shape != (B, A):
        raise ValueError(f"{who}: det is fp32 [{batch_size}, A, 6] and track_id int64 [{batch_size}, A], got {det.shape} and "
                         f"{track_id.shape}")
    if gt_box.shape != (B, G, 4) or gt_label.shape != (B, G) or gt_id.shape != (B, G) or not 0 <= G <= DAGR_SCORE_MAX_GT or \
            any(t.shape != (B, G if w is None else w) for t, w in zip(tables, widths)):
        more = "".join(f", {name} int64 [{B}, {'G' if w is None else w}]" for name, w in zip(names, widths))
        got = ", ".join(str(a.shape) for a in [gt_box, gt_label, gt_id] + tables)
        raise ValueError(f"{who}: the ground truth is gt_box fp32 [{B}, G, 4], gt_label int32 [{B}, G] and gt_id int64 "
                         f"[{B}, G] with G <= DAGR_SCORE_MAX_GT = {DAGR_SCORE_MAX_GT}{more}, got {got}")
    if boxes == "track":
        if track_box is None:
            raise ValueError(f"{who}: score boxes = 'track' needs the step's track_box")
        boxes = np.asarray(track_box, np.float32)
    else:
        boxes = det[..., :4]
    with np.errstate(all="ignore"):
        labels = det[..., 5].astype(np.int32)
    n = np.clip(np.broadcast_to(np.asarray(n_keep, np.int64).reshape(-1), (B,)), 0, A)
    n_gt = np.full(B, G, np.int64) if n_gt is None else np.broadcast_to(np.asarray(n_gt, np.int64).reshape(-1), (B,))
    return (track_id, boxes, labels, gt_box, gt_label, gt_id, n, np.minimum(n_gt, G), *tables)


def _lane_hypotheses(track_id, n, first_carriers=False):
    """A lane's hypotheses and how many rows have an id: of ``track_id`` int64 ``[A]`` the rows below ``n`` with an id, in
    row order, cut at ``DAGR_TRACK_MAX_DETS``; with ``first_carriers`` of those only the first row that carries an id (a
    carrier behind the cut is none)."""
    with_id = [i for i in range(n) if track_id[i] != 0]
    hyp = with_id[:DAGR_TRACK_MAX_DETS]
    if first_carriers:
        first = {}
        for i in hyp:
            first.setdefault(int(track_id[i]), i)
        hyp = list(first.values())
    return hyp, len(with_id)


def _lane_scored_rows(gt_id, gt_match, ng, score_ids):
    """The rows of a lane that count behind the scorer, as ``[(row, slot)]`` in row order: a row below ``ng`` that the
    scorer scored (its ``gt_match`` is not -1, its identity positive) and whose identity ``score_ids``, the scorer's id
    table of the lane, holds -- at the first slot that does."""
    rows = []
    for g in range(ng):
        known = np.flatnonzero(score_ids == gt_id[g]) if gt_match[g] != -1 and gt_id[g] > 0 else []
        if len(known):
            rows.append((g, int(known[0])))
    return rows


class ScoreDefinition:
    """The scorer of the module docstring in numpy -- this project's statement of the CLEAR-MOT counts with a greedy
    matcher: ``step(det, n_keep, track_id, gt_box, gt_label, gt_id, n_gt=None, track_box=None)`` is one scored step of every
    lane and returns ``(gt_match int64 [B, G], gt_flags int32 [B, G])``; given ``out=(gt_match, gt_flags)`` it writes into
    them, so that the rows at and behind ``n_gt[b]`` and the rows of a skipped lane are left as they were (otherwise they
    are zero).  The state is the table's arrays, one per name of ``SCORE_OBJECT_FIELDS`` over ``[B, max_objects]``,
    ``n_objects`` int64 ``[B]`` and ``counters``, a dict of one int64 ``[B]`` array per name of ``SCORE_COUNTERS``.
    ``events`` counts what has happened so far -- matches, misses, false positives, switches, fragmentations, kept pairs,
    keep candidates that lost their hypothesis, new objects, unscored ground-truth rows, rows without an id -- so that a
    test can tell a run that exercises every rule from one that does not.  The yardstick of ``dagr_stream_score``; nothing
    on the device path calls it."""

    def __init__(self, batch_size, score=True):
        self.B = int(batch_size)
        self.options = _score_options(score, True, True, "ScoreDefinition")       # (what it scores is the caller's business)
        if self.options is None:
            raise ValueError("ScoreDefinition: score = None is a stream that does not score")
        self.reset()

    def reset(self):
        B, M = self.B, self.options["max_objects"]
        for name in SCORE_OBJECT_FIELDS:
            setattr(self, name, np.full((B, M), -1 if name == "seen_step" else 0, np.int64))
        self.n_objects = np.zeros(B, np.int64)
        self.counters = {name: np.zeros(B, np.int64) for name in SCORE_COUNTERS}
        self.events = dict(matched=0, missed=0, false_pos=0, switched=0, fragmented=0, kept=0, keep_lost=0, new_objects=0,
                           unscored_gt=0, rows_without_id=0)

    def step(self, det, n_keep, track_id, gt_box, gt_label, gt_id, n_gt=None, track_box=None, out=None):
        f, o = np.float32, self.options
        track_id, boxes, all_labels, gt_box, gt_label, gt_id, n_rows, n_gt = _labelled_step(
            "ScoreDefinition", self.B, o["boxes"], det, n_keep, track_id, gt_box, gt_label, gt_id, n_gt, track_box)
        B, G = gt_label.shape
        gt_match, gt_flags = out if out is not None else (np.zeros((B, G), np.int64), np.zeros((B, G), np.int32))
        thr, M, c, ev = f(o["iou"]), o["max_objects"], self.counters, self.events
        for b in range(B):
            if n_gt[b] < 0:                                        # no labels at this instant: not one byte changes
                continue
            n, ng, steps, labels = int(n_rows[b]), int(n_gt[b]), int(c["steps"][b]), all_labels[b]
            hyp, n_with_id = _lane_hypotheses(track_id[b], n)                      # 1: the hypotheses
            ev["rows_without_id"] += n - n_with_id
            c["unscored_hyp"][b] += n_with_id - len(hyp)
            slot, earlier = {}, set()                                             # 2: the slots
            for g in range(ng):
                ident = int(gt_id[b, g])
                known = np.flatnonzero(self.id[b, :self.n_objects[b]] == ident)
                if ident > 0 and ident not in earlier and (len(known) or self.n_objects[b] < M):
                    if len(known):
                        slot[g] = int(known[0])
                    else:
                        slot[g] = int(self.n_objects[b])
                        self.id[b, slot[g]] = ident
                        self.n_objects[b] += 1
                        ev["new_objects"] += 1
                else:
                    c["unscored_gt"][b] += 1
                    ev["unscored_gt"] += 1
                    gt_match[b, g], gt_flags[b, g] = -1, 0
                earlier.add(ident)
            free = [True] * len(hyp)
            got = {}                                                              # row g -> (hypothesis, iou, kept)
            for g, s in slot.items():                                             # 3: keep
                prev = int(self.prev_hyp[b, s])
                if self.seen_step[b, s] != steps - 1 or prev == 0:
                    continue
                first = next((p for p, i in enumerate(hyp) if track_id[b, i] == prev), None)
                v = None if first is None else TrackDefinition.iou(gt_box[b, g], boxes[b, hyp[first]])
                if first is not None and free[first] and labels[hyp[first]] == gt_label[b, g] and v >= thr:
                    free[first] = False
                    got[g] = (first, v, True)
                else:
                    ev["keep_lost"] += 1
            for g in slot:                                                        # 4: match
                if g in got:
                    continue
                best, best_p = None, None
                for p, i in enumerate(hyp):
                    if not free[p] or labels[i] != gt_label[b, g]:
                        continue
                    v = TrackDefinition.iou(gt_box[b, g], boxes[b, i])
                    if v >= thr and (best is None or v > best):                   # (a NaN IoU matches nothing; ties: lowest row)
                        best, best_p = v, p
                if best_p is not None:
                    free[best_p] = False
                    got[g] = (best_p, best, False)
            for g, s in slot.items():                                             # 5: count
                c["gt"][b] += 1
                self.present[b, s] += 1
                self.seen_step[b, s] = steps
                if g not in got:
                    c["miss"][b] += 1
                    ev["missed"] += 1
                    self.prev_hyp[b, s] = 0
                    gt_match[b, g], gt_flags[b, g] = 0, 0
                    continue
                p, v, kept = got[g]
                h = int(track_id[b, hyp[p]])
                flags = SCORE_KEPT if kept else 0
                c["match"][b] += 1
                c["iou_q"][b] += int(np.rint(f(v * f(SCORE_IOU_ONE))))
                c["kept"][b] += int(kept)
                if self.last_hyp[b, s] != 0 and self.last_hyp[b, s] != h:
                    flags |= SCORE_SWITCH
                    c["switch"][b] += 1
                    self.switches[b, s] += 1
                    ev["switched"] += 1
                if self.tracked[b, s] > 0 and self.prev_hyp[b, s] == 0:
                    flags |= SCORE_FRAG
                    c["frag"][b] += 1
                    self.frags[b, s] += 1
                    ev["fragmented"] += 1
                self.tracked[b, s] += 1
                self.last_hyp[b, s] = self.prev_hyp[b, s] = h
                gt_match[b, g], gt_flags[b, g] = h, flags
                ev["matched"] += 1
                ev["kept"] += int(kept)
            c["hyp"][b] += len(hyp)
            c["false_pos"][b] += sum(free)
            ev["false_pos"] += sum(free)
            c["steps"][b] += 1
        return gt_match, gt_flags

    def objects(self):
        """Per lane the object table as a ``SCORE_OBJECT_DTYPE`` array in order of first appearance (what
        ``EventStream.scored_objects()`` returns)."""
        return [objects_from_arrays(int(self.n_objects[b]), *(getattr(self, name)[b] for name in SCORE_OBJECT_FIELDS))
                for b in range(self.B)]


def objects_from_arrays(n, *fields):
    """One lane's object table -> its first ``n`` slots as a ``SCORE_OBJECT_DTYPE`` array; ``fields`` in the order of
    ``SCORE_OBJECT_FIELDS``."""
    out = np.zeros(n, SCORE_OBJECT_DTYPE)
    for name, a in zip(SCORE_OBJECT_FIELDS, fields):
        out[name] = a[:n]
    return out


def score_summary(counters, objects):
    """``counters`` (a dict of int64 ``[B]`` per name of ``SCORE_COUNTERS``) and ``objects`` (per lane a
    ``SCORE_OBJECT_DTYPE`` array) -> ``dict(lanes=[...], total=...)``, each entry a dict of ``mota``, ``motp``, ``precision``,
    ``recall`` (floats, ``nan`` where the denominator is 0), ``gt``, ``match``, ``miss``, ``false_pos``, ``switch``, ``frag``,
    ``objects``, ``mostly_tracked`` and ``mostly_lost`` (ints).  Plain host code."""
    def one(c, tables):
        ratio = lambda a, b: float(a) / float(b) if b else float("nan")            # noqa: E731
        present = np.concatenate([t["present"] for t in tables]) if tables else np.zeros(0, np.int64)
        tracked = np.concatenate([t["tracked"] for t in tables]) if tables else np.zeros(0, np.int64)
        # tracked / present >= 0.8 and <= 0.2 in integers; an object that was never scored (present 0) is neither
        return dict(mota=1.0 - ratio(c["miss"] + c["false_pos"] + c["switch"], c["gt"]) if c["gt"] else float("nan"),
                    motp=ratio(c["iou_q"], SCORE_IOU_ONE * c["match"]),
                    precision=ratio(c["match"], c["match"] + c["false_pos"]), recall=ratio(c["match"], c["gt"]),
                    gt=c["gt"], match=c["match"], miss=c["miss"], false_pos=c["false_pos"], switch=c["switch"], frag=c["frag"],
                    objects=int(len(present)),
                    mostly_tracked=int(np.sum((present > 0) & (5 * tracked >= 4 * present))),
                    mostly_lost=int(np.sum((present > 0) & (5 * tracked <= present))))
    B = len(objects)
    per_lane = [{k: int(np.asarray(counters[k]).reshape(-1)[b]) for k in SCORE_COUNTERS} for b in range(B)]
    total = {k: sum(c[k] for c in per_lane) for k in SCORE_COUNTERS}
    return dict(lanes=[one(per_lane[b], [objects[b]]) for b in range(B)], total=one(total, list(objects)))


DAGR_ASSIGN_MAX = DEFINES["DAGR_ASSIGN_MAX"]
IDENTITY_DEFAULTS = dict(max_tracks=256)
IDENTITY_WORDS = ("n_tracks", "n_objects", "gt_frames", "hyp_frames", "dup_hyp", "unlisted_hyp", "pairs", "steps")
IDENTITY_RESULT = ("idtp", "idfn", "idfp", "gt_frames", "hyp_frames", "n_objects", "n_tracks", "dup_hyp", "unlisted_hyp")


def assign_max_weight_definition(w, stats=None):
    """The maximum-weight assignment of the module docstring in numpy: ``w`` int ``[n, m]``, ``w >= 0``, ``n, m`` in
    0 .. ``DAGR_ASSIGN_MAX`` -> ``(total, row_col)``, a Python int and int64 ``[n]`` (a column, or -1: no pair, or a pair of
    weight 0).  ``total`` is unique, ``row_col`` is one pairing that reaches it (``check_assignment``).  ``stats``, a dict,
    gets ``steps`` (path steps) and ``transposed``.  The yardstick of ``dagr_assign_max_weight``."""
    w = np.asarray(w)
    if w.ndim != 2 or not np.issubdtype(w.dtype, np.integer) or max(w.shape) > DAGR_ASSIGN_MAX:
        raise ValueError(f"assign_max_weight_definition: w is an int array [n, m] with n, m <= DAGR_ASSIGN_MAX = "
                         f"{DAGR_ASSIGN_MAX}, got {w.dtype} {w.shape}")
    if w.size and w.min() < 0:
        raise ValueError("assign_max_weight_definition: w must be >= 0")
    n, m = w.shape
    row_col = np.full(n, -1, np.int64)
    transposed = n > m
    if stats is not None:
        stats.update(steps=0, transposed=transposed)
    if n == 0 or m == 0:
        return 0, row_col
    a = (w.T if transposed else w).astype(np.int64)
    cost = -a
    R, C = cost.shape
    inf = np.iinfo(np.int64).max
    u, v = np.zeros(R + 1, np.int64), np.zeros(C + 1, np.int64)        # 1-based; row 0 / column 0 are the path's root
    p, way = np.zeros(C + 1, np.int64), np.zeros(C + 1, np.int64)      # p[j]: the row of column j, 0: free
    steps = 0
    for i in range(1, R + 1):
        p[0], j0 = i, 0
        minv, used = np.full(C + 1, inf, np.int64), np.zeros(C + 1, bool)
        while True:
            used[j0] = True
            i0 = p[j0]
            free = ~used                                                # (column 0 is used from the first step on)
            cur = cost[i0 - 1] - u[i0] - v[1:]
            better = free[1:] & (cur < minv[1:])
            minv[1:][better], way[1:][better] = cur[better], j0
            cand = np.where(free[1:], minv[1:], inf)
            j1 = int(np.argmin(cand)) + 1                               # the lowest column of equals
            delta = cand[j1 - 1]
            u[p[used]] += delta                                         # (the rows of the used columns are distinct)
            v[used] -= delta
            minv[free] -= delta
            j0 = j1
            steps += 1
            if p[j0] == 0:
                break
        while j0:
            j1 = int(way[j0])
            p[j0] = p[j1]
            j0 = j1
    total = 0
    for j in range(1, C + 1):
        if p[j] and a[p[j] - 1, j - 1] > 0:
            r, c = int(p[j]) - 1, j - 1
            total += int(a[r, c])
            if transposed:
                row_col[c] = r
            else:
                row_col[r] = c
    if stats is not None:
        stats["steps"] = steps
    return total, row_col


def check_assignment(w, total, row_col):
    """Whether ``row_col`` is a right answer for ``w`` with the total ``total``: every entry -1 or a column in range, no
    column twice, no pair of weight 0, and the pairs sum to ``total``.  Returns None or what is wrong, in words."""
    w, row_col = np.asarray(w), np.asarray(row_col)
    n, m = w.shape
    if row_col.shape != (n,):
        return f"row_col has shape {row_col.shape}, not ({n},)"
    rows = np.flatnonzero(row_col != -1)
    cols = row_col[rows]
    if len(cols) and (cols.min() < 0 or cols.max() >= m):
        return "a column out of range"
    if len(set(cols.tolist())) != len(cols):
        return "a column is paired twice"
    weights = w[rows, cols].astype(np.int64) if len(rows) else np.zeros(0, np.int64)
    if (weights <= 0).any():
        return "a pair of weight 0 is listed"
    if int(weights.sum()) != int(total):
        return f"the pairs sum to {int(weights.sum())}, not to {int(total)}"
    return None


def _identity_options(identity, score_options, who):
    """``identity=`` of a scoring stream, checked: None (off) or ``dict(max_tracks=)``; ``score_options`` is what
    ``_score_options`` returned.  Refusals by name."""
    opt = _options(identity, "identity", IDENTITY_DEFAULTS, who)
    if opt is None:
        return None
    if score_options is None:
        raise ValueError(f"{who}: identity= needs score= (it counts the rows the scorer scored)")
    if not _is_int(opt["max_tracks"]) or not 1 <= int(opt["max_tracks"]) <= DAGR_ASSIGN_MAX:
        raise ValueError(f"{who}: identity max_tracks = {opt['max_tracks']!r} must be an int in 1..DAGR_ASSIGN_MAX = "
                         f"{DAGR_ASSIGN_MAX}")
    return dict(max_tracks=int(opt["max_tracks"]))


class IdentityDefinition:
    """The identity state of the module docstring in numpy: ``step(det, n_keep, track_id, gt_box, gt_label, gt_id, n_gt,
    gt_match, score_ids, track_box=None)`` is one step of every lane behind the scorer's on the same arrays -- ``gt_match``
    int64 ``[B, G]`` is what that step wrote, ``score_ids`` int64 ``[B, max_objects]`` the scorer's id table after it --, and
    ``solve()`` returns the dict of ``IDENTITY_RESULT`` (int64 ``[B]`` each) plus ``obj_track`` int64 ``[B, max_objects]``.
    The state is ``track_id``, ``track_len`` int64 ``[B, max_tracks]``, ``obj_len`` int64 ``[B, max_objects]``, ``overlap``
    int32 ``[B, max_objects, max_tracks]`` and ``words``, a dict of one int64 ``[B]`` array per name of ``IDENTITY_WORDS``.
    ``events`` counts what has happened so far -- pairs, duplicate ids, unlisted hypotheses, new columns, ground-truth rows
    skipped, lanes skipped, label mismatches, NaN IoUs, hypotheses shared by two objects at a step -- so that a test can
    tell a run that exercises every rule from one that does not.  The yardstick of ``dagr_stream_identity`` and
    ``dagr_stream_identity_solve``; nothing on the device path calls it."""

    def __init__(self, batch_size, identity=True, score=True):
        self.B = int(batch_size)
        self.score = _score_options(score, True, True, "IdentityDefinition")
        if self.score is None:
            raise ValueError("IdentityDefinition: score = None is a stream that does not score")
        self.options = _identity_options(identity, self.score, "IdentityDefinition")
        if self.options is None:
            raise ValueError("IdentityDefinition: identity = None is a stream without it")
        self.reset()

    def reset(self):
        B, M, T = self.B, self.score["max_objects"], self.options["max_tracks"]
        self.track_id, self.track_len = np.zeros((B, T), np.int64), np.zeros((B, T), np.int64)
        self.obj_len, self.overlap = np.zeros((B, M), np.int64), np.zeros((B, M, T), np.int32)
        self.words = {name: np.zeros(B, np.int64) for name in IDENTITY_WORDS}
        self.events = dict(pairs=0, duplicates=0, unlisted=0, new_columns=0, rows_skipped=0, lanes_skipped=0,
                           label_mismatch=0, nan_iou=0, shared_hyp=0)

    def step(self, det, n_keep, track_id, gt_box, gt_label, gt_id, n_gt, gt_match, score_ids, track_box=None):
        M, T, w, ev = self.score["max_objects"], self.options["max_tracks"], self.words, self.events
        track_id, boxes, all_labels, gt_box, gt_label, gt_id, n_rows, n_gt, gt_match, score_ids = _labelled_step(
            "IdentityDefinition", self.B, self.score["boxes"], det, n_keep, track_id, gt_box, gt_label, gt_id, n_gt, track_box,
            gt_match=(gt_match, None), score_ids=(score_ids, M))
        thr = np.float32(self.score["iou"])
        for b in range(self.B):
            if n_gt[b] < 0:                                        # no labels at this instant: not one byte changes
                ev["lanes_skipped"] += 1
                continue
            n, ng, labels = int(n_rows[b]), int(n_gt[b]), all_labels[b]
            hyp, n_with_id = _lane_hypotheses(track_id[b], n, first_carriers=True)  # 1: the hypotheses
            duplicates = min(n_with_id, DAGR_TRACK_MAX_DETS) - len(hyp)
            w["dup_hyp"][b] += duplicates
            ev["duplicates"] += duplicates
            w["hyp_frames"][b] += len(hyp)
            col = {}
            for i in hyp:                                                          # 2: the columns
                ident = int(track_id[b, i])
                known = np.flatnonzero(self.track_id[b, :w["n_tracks"][b]] == ident)
                if len(known):
                    col[i] = int(known[0])
                elif w["n_tracks"][b] < T:
                    col[i] = int(w["n_tracks"][b])
                    self.track_id[b, col[i]] = ident
                    w["n_tracks"][b] += 1
                    ev["new_columns"] += 1
                else:
                    w["unlisted_hyp"][b] += 1
                    ev["unlisted"] += 1
                    continue
                self.track_len[b, col[i]] += 1
            slot = dict(_lane_scored_rows(gt_id[b], gt_match[b], ng, score_ids[b]))     # 3: the rows
            ev["rows_skipped"] += ng - len(slot)
            w["gt_frames"][b] += len(slot)
            for s in slot.values():
                self.obj_len[b, s] += 1
                w["n_objects"][b] = max(int(w["n_objects"][b]), s + 1)
            hit = set()
            for g, s in slot.items():                                              # 4: the pairs
                for i, c in col.items():
                    if labels[i] != gt_label[b, g]:
                        ev["label_mismatch"] += 1
                        continue
                    v = TrackDefinition.iou(gt_box[b, g], boxes[b, i])
                    ev["nan_iou"] += int(v != v)
                    if v >= thr:
                        self.overlap[b, s, c] += 1
                        w["pairs"][b] += 1
                        ev["pairs"] += 1
                        ev["shared_hyp"] += int(i in hit)
                        hit.add(i)
            w["steps"][b] += 1

    def solve(self, stats=None):
        """The assignment on every lane's ``overlap[:n_objects, :n_tracks]``: the dict of ``IDENTITY_RESULT`` (int64 ``[B]``)
        plus ``obj_track`` int64 ``[B, max_objects]`` (the paired track id, 0: none).  ``stats``, a list, gets one dict per
        lane (``assign_max_weight_definition``)."""
        B, M, w = self.B, self.score["max_objects"], self.words
        out = {name: np.zeros(B, np.int64) for name in IDENTITY_RESULT}
        out["obj_track"] = np.zeros((B, M), np.int64)
        for b in range(B):
            n, m = int(w["n_objects"][b]), int(w["n_tracks"][b])
            st = {}
            total, row_col = assign_max_weight_definition(self.overlap[b, :n, :m], st)
            if stats is not None:
                stats.append(st)
            out["idtp"][b] = total
            out["idfn"][b], out["idfp"][b] = w["gt_frames"][b] - total, w["hyp_frames"][b] - total
            for name in IDENTITY_RESULT[3:]:
                out[name][b] = w[name][b]
            paired = row_col >= 0
            out["obj_track"][b, :n][paired] = self.track_id[b, row_col[paired]]
        return out


def check_identity(overlap, track_id, result, b):
    """Whether lane ``b`` of a solve's ``result`` is a right answer for the lane's ``overlap`` int32 ``[max_objects,
    max_tracks]`` and ``track_id`` int64 ``[max_tracks]``: ``obj_track`` names listed tracks, none twice, only pairs that
    overlap, and they sum to ``idtp``.  Returns None or what is wrong, in words."""
    n, m = int(result["n_objects"][b]), int(result["n_tracks"][b])
    obj_track = np.asarray(result["obj_track"][b])
    if obj_track[n:].any():
        return "an object behind n_objects is paired"
    row_col = np.full(n, -1, np.int64)
    for s in np.flatnonzero(obj_track[:n]):
        known = np.flatnonzero(np.asarray(track_id[:m]) == obj_track[s])
        if len(known) != 1:
            return f"object {s} is paired with track {obj_track[s]}, which is not listed once"
        row_col[s] = known[0]
    return check_assignment(np.asarray(overlap)[:n, :m], result["idtp"][b], row_col)


def identity_summary(result):
    """A solve's ``result`` (the dict of int64 ``[B]`` per name of ``IDENTITY_RESULT``) -> ``dict(lanes=[...], total=...)``,
    each entry a dict of ``idf1`` (``2 idtp / (gt_frames + hyp_frames)``), ``idp`` (``idtp / hyp_frames``), ``idr``
    (``idtp / gt_frames``) -- floats, ``nan`` where the denominator is 0 -- and ``idtp``, ``idfn``, ``idfp``, ``gt_frames``,
    ``hyp_frames``, ``objects``, ``tracks`` (ints).  The total sums the lanes' integers.  Plain host code."""
    def one(c):
        ratio = lambda a, b: float(a) / float(b) if b else float("nan")            # noqa: E731
        return dict(idf1=ratio(2 * c["idtp"], c["gt_frames"] + c["hyp_frames"]), idp=ratio(c["idtp"], c["hyp_frames"]),
                    idr=ratio(c["idtp"], c["gt_frames"]), idtp=c["idtp"], idfn=c["idfn"], idfp=c["idfp"],
                    gt_frames=c["gt_frames"], hyp_frames=c["hyp_frames"], objects=c["n_objects"], tracks=c["n_tracks"])
    B = len(np.asarray(result["idtp"]).reshape(-1))
    per_lane = [{k: int(np.asarray(result[k]).reshape(-1)[b]) for k in IDENTITY_RESULT} for b in range(B)]
    total = {k: sum(c[k] for c in per_lane) for k in IDENTITY_RESULT}
    return dict(lanes=[one(c) for c in per_lane], total=one(total))


DAGR_HOTA_MAX_INSTANTS = DEFINES["DAGR_HOTA_MAX_INSTANTS"]
DAGR_HOTA_MAX_STATE_BYTES = DEFINES["DAGR_HOTA_MAX_STATE_BYTES"]
HOTA_THRESHOLDS = DEFINES["DAGR_HOTA_THRESHOLDS"]        # alpha = k / 20, k = 1 .. 19
HOTA_DEFAULTS = dict(max_instants=1200)
HOTA_WORDS = ("instants", "dropped_instants", "rows", "columns")
HOTA_COUNTERS = ("tp", "fn", "fp", "loc_q")             # int64 [B, 19] each
HOTA_SUMS = ("ass", "re", "pr")                         # fp64 [B, 19] each


def _hota_options(hota, identity_options, who):
    """``hota=`` of an identity stream, checked: None (off) or ``dict(max_instants=)``; ``identity_options`` is what
    ``_identity_options`` returned.  Refusals by name."""
    opt = _options(hota, "hota", HOTA_DEFAULTS, who)
    if opt is None:
        return None
    if identity_options is None:
        raise ValueError(f"{who}: hota= needs identity= (its participants are the rows and columns of the identity state)")
    if not _is_int(opt["max_instants"]) or not 1 <= int(opt["max_instants"]) <= DAGR_HOTA_MAX_INSTANTS:
        raise ValueError(f"{who}: hota max_instants = {opt['max_instants']!r} must be an int in 1..DAGR_HOTA_MAX_INSTANTS = "
                         f"{DAGR_HOTA_MAX_INSTANTS}")
    return dict(max_instants=int(opt["max_instants"]))


def hota_similarity(gt_box, gt_label, hyp_box, hyp_label):
    """``q`` int64 ``[n, m]`` of the module docstring: ``rint(fp32(iou) * 2**20)`` with ``TrackDefinition.iou``'s operations
    (the ground-truth box is ``a``), 0 where the labels differ and where the IoU is NaN or outside (0, 1]."""
    f = np.float32
    a, b = np.asarray(gt_box, f).reshape(-1, 1, 4), np.asarray(hyp_box, f).reshape(1, -1, 4)
    same = np.asarray(gt_label, np.int32).reshape(-1, 1) == np.asarray(hyp_label, np.int32).reshape(1, -1)
    with np.errstate(all="ignore"):
        iw = np.minimum(a[..., 2], b[..., 2]) - np.maximum(a[..., 0], b[..., 0])
        ih = np.minimum(a[..., 3], b[..., 3]) - np.maximum(a[..., 1], b[..., 1])
        inter = np.where((iw > 0) & (ih > 0), iw * ih, f(0))
        union = ((a[..., 2] - a[..., 0]) * (a[..., 3] - a[..., 1]) + (b[..., 2] - b[..., 0]) * (b[..., 3] - b[..., 1])) - inter
        v = inter / union
        q = np.rint(v * f(SCORE_IOU_ONE))
    assert v.dtype == f
    return np.where(same & (v > 0) & (v <= 1), q, f(0)).astype(np.int64)


class HotaDefinition:
    """HOTA's state of the module docstring in numpy: ``step(det, n_keep, track_id, gt_box, gt_label, gt_id, n_gt, gt_match,
    score_ids, columns, track_box=None)`` is pass 1 and the append for one step of every lane, behind the identity step on
    the same arrays -- ``gt_match`` int64 ``[B, G]`` and ``score_ids`` int64 ``[B, max_objects]`` as ``IdentityDefinition.step``
    takes them, ``columns`` int64 ``[B, max_tracks]`` the identity state's ``track_id`` table after its step --, and
    ``solve()`` is pass 2 and the reduce: a dict of ``tp``, ``fn``, ``fp``, ``loc_q`` (int64 ``[B, 19]``), ``ass``, ``re``,
    ``pr`` (fp64 ``[B, 19]``), ``mc`` (int32 ``[B, 19, max_objects, max_tracks]``) and one int64 ``[B]`` per name of
    ``HOTA_WORDS``.  The state is ``pmc`` int64 ``[B, max_objects, max_tracks]``, ``gc`` int64 ``[B, max_objects]``, ``tc``
    int64 ``[B, max_tracks]``, ``words`` and ``log``, per lane a list of ``dict(slot, col, gt_box, gt_label, hyp_box,
    hyp_label)``.  ``events`` counts what has happened so far -- instants logged and dropped, lanes skipped, instants
    without rows and without columns, pairs whose labels differ, NaN IoUs, and after a solve the matched pairs, the
    instants where the alignment score decided (the pairing on ``q`` alone is another) and the matrices with more rows than
    columns and the reverse -- so that a test can tell a run that exercises every rule from one that does not.  The
    yardstick of ``dagr_stream_hota`` and ``dagr_stream_hota_solve``; nothing on the device path calls it."""

    def __init__(self, batch_size, hota=True, identity=True, score=True):
        self.B = int(batch_size)
        self.score = _score_options(score, True, True, "HotaDefinition")
        if self.score is None:
            raise ValueError("HotaDefinition: score = None is a stream that does not score")
        self.identity = _identity_options(identity, self.score, "HotaDefinition")
        self.options = _hota_options(hota, self.identity, "HotaDefinition")
        if self.options is None:
            raise ValueError("HotaDefinition: hota = None is a stream without it")
        self.reset()

    def reset(self):
        B, M, T = self.B, self.score["max_objects"], self.identity["max_tracks"]
        self.pmc, self.gc, self.tc = np.zeros((B, M, T), np.int64), np.zeros((B, M), np.int64), np.zeros((B, T), np.int64)
        self.words = {name: np.zeros(B, np.int64) for name in HOTA_WORDS}
        self.log = [[] for _ in range(B)]
        self.events = dict(logged=0, dropped=0, lanes_skipped=0, no_rows=0, no_columns=0, label_mismatch=0, nan_iou=0,
                           matched=0, alignment_decides=0, tall=0, wide=0)

    def step(self, det, n_keep, track_id, gt_box, gt_label, gt_id, n_gt, gt_match, score_ids, columns, track_box=None):
        M, T, w, ev = self.score["max_objects"], self.identity["max_tracks"], self.words, self.events
        track_id, boxes, all_labels, gt_box, gt_label, gt_id, n_rows, n_gt, gt_match, score_ids, columns = _labelled_step(
            "HotaDefinition", self.B, self.score["boxes"], det, n_keep, track_id, gt_box, gt_label, gt_id, n_gt, track_box,
            gt_match=(gt_match, None), score_ids=(score_ids, M), columns=(columns, T))
        for b in range(self.B):
            if n_gt[b] < 0:                                        # no labels at this instant: not one byte changes
                ev["lanes_skipped"] += 1
                continue
            if w["instants"][b] >= self.options["max_instants"]:   # a full log: nothing but the count of what is left out
                w["dropped_instants"][b] += 1
                ev["dropped"] += 1
                continue
            n, ng, labels = int(n_rows[b]), int(n_gt[b]), all_labels[b]
            hyp, col = [], []                                      # the hypotheses with a column, in row order
            for i in _lane_hypotheses(track_id[b], n, first_carriers=True)[0]:
                known = np.flatnonzero(columns[b] == track_id[b, i])
                if len(known):
                    hyp.append(i)
                    col.append(int(known[0]))
            scored = _lane_scored_rows(gt_id[b], gt_match[b], ng, score_ids[b])   # the ground-truth rows with a slot
            rows = [g for g, _ in scored]
            slot, col = np.asarray([s for _, s in scored], np.int64), np.asarray(col, np.int64)
            entry = dict(slot=slot, col=col, gt_box=gt_box[b, rows].copy(), gt_label=gt_label[b, rows].copy(),
                         hyp_box=boxes[b, hyp].copy(), hyp_label=labels[hyp].copy())
            q = hota_similarity(entry["gt_box"], entry["gt_label"], entry["hyp_box"], entry["hyp_label"])
            ev["label_mismatch"] += int((entry["gt_label"].reshape(-1, 1) != entry["hyp_label"].reshape(1, -1)).sum())
            ev["nan_iou"] += int(np.isnan(entry["gt_box"]).any(-1).sum() * len(hyp) + np.isnan(entry["hyp_box"]).any(-1).sum() * len(rows))
            rs, cs = q.sum(1, keepdims=True), q.sum(0, keepdims=True)
            den = np.where(q > 0, rs + cs - q, 1)
            self.pmc[b][np.ix_(slot, col)] += np.where(q > 0, (q << 20) // den, 0)      # (distinct slots, distinct columns)
            self.gc[b, slot] += 1
            self.tc[b, col] += 1
            self.log[b].append(entry)
            w["instants"][b] += 1
            w["rows"][b] += len(rows)
            w["columns"][b] += len(hyp)
            ev["logged"] += 1
            ev["no_rows"] += int(len(rows) == 0)
            ev["no_columns"] += int(len(hyp) == 0)

    def weights(self, b, entry):
        """``(q int64 [n, m], w int32 [n, m])`` of a logged instant of lane ``b`` under the tables as they are now."""
        q = hota_similarity(entry["gt_box"], entry["gt_label"], entry["hyp_box"], entry["hyp_label"])
        pmc = self.pmc[b][np.ix_(entry["slot"], entry["col"])]
        both = (self.gc[b, entry["slot"]].reshape(-1, 1) + self.tc[b, entry["col"]].reshape(1, -1)) << 20
        gq = np.where(pmc > 0, (pmc << 20) // np.where(pmc > 0, both - pmc, 1), 0)
        return q, ((gq * q) >> 10).astype(np.int32)

    def solve(self, pairings=None):
        """Pass 2 on the log with the tables as they are now, and the reduce (the class docstring lists the result).
        Changes no table.  ``pairings``, a list, gets per lane the list of every instant's ``row_col``."""
        B, M, T, K, ev = self.B, self.score["max_objects"], self.identity["max_tracks"], HOTA_THRESHOLDS, self.events
        out = {name: np.zeros((B, K), np.int64) for name in HOTA_COUNTERS}
        out.update({name: np.zeros((B, K), np.float64) for name in HOTA_SUMS})
        out.update({name: self.words[name].copy() for name in HOTA_WORDS})
        out["mc"] = np.zeros((B, K, M, T), np.int32)
        for b in range(B):
            lane_pairs = []
            for entry in self.log[b]:
                q, w = self.weights(b, entry)
                n, m = q.shape
                _, row_col = assign_max_weight_definition(w)
                lane_pairs.append(row_col)
                ev["tall"] += int(n > m)
                ev["wide"] += int(m > n)
                if n and m and not np.array_equal(row_col, assign_max_weight_definition(q.astype(np.int32))[1]):
                    ev["alignment_decides"] += 1
                tps = np.zeros(K, np.int64)
                for g in np.flatnonzero(row_col >= 0):
                    i = int(row_col[g])
                    ev["matched"] += 1
                    for k in range(1, K + 1):
                        if 20 * int(q[g, i]) >= k << 20:           # exact: alpha = k / 20, no epsilon
                            tps[k - 1] += 1
                            out["loc_q"][b, k - 1] += int(q[g, i])
                            out["mc"][b, k - 1, entry["slot"][g], entry["col"][i]] += 1
                out["tp"][b] += tps
                out["fn"][b] += n - tps
                out["fp"][b] += m - tps
            if pairings is not None:
                pairings.append(lane_pairs)
            for k in range(K):                                     # the reduce: one division, then one multiplication
                s, c = np.nonzero(out["mc"][b, k])
                mc = out["mc"][b, k, s, c].astype(np.float64)
                gc, tc = self.gc[b, s].astype(np.float64), self.tc[b, c].astype(np.float64)
                out["ass"][b, k] = np.sum(mc * (mc / (gc + tc - mc)))
                out["re"][b, k] = np.sum(mc * (mc / gc))
                out["pr"][b, k] = np.sum(mc * (mc / tc))
        return out


def hota_summary(result):
    """A solve's ``result`` (``tp``, ``fn``, ``fp``, ``loc_q`` int64 ``[B, 19]``, ``ass``, ``re``, ``pr`` fp64 ``[B, 19]``,
    ``instants`` and ``dropped_instants`` int64 ``[B]``) -> ``dict(lanes=[...], total=...)``.  Each entry has per threshold
    (``alphas``: a dict of 19-entry lists, alpha = 0.05 .. 0.95) ``deta = tp / max(1, tp + fn + fp)``, ``detre``, ``detpr``,
    ``assa = ass / max(1, tp)``, ``assre``, ``asspr``, ``loca = loc_q / (2**20 * tp)`` (``nan`` where ``tp`` is 0) and ``hota =
    sqrt(deta * assa)``, under the same names their means over the 19 thresholds (``loca``: over the thresholds with a TP,
    ``nan`` when there is none), and ``tp``, ``fn``, ``fp`` (lists), ``instants``, ``dropped_instants`` (ints).  The total sums
    the lanes' integers and the lanes' fp64 sums before it divides.  Plain host code."""
    def one(c):
        tp, fn, fp = (c[k].astype(np.float64) for k in ("tp", "fn", "fp"))
        least = np.maximum(1.0, tp)
        with np.errstate(all="ignore"):
            a = dict(deta=tp / np.maximum(1.0, tp + fn + fp), detre=tp / np.maximum(1.0, tp + fn),
                     detpr=tp / np.maximum(1.0, tp + fp), assa=c["ass"] / least, assre=c["re"] / least, asspr=c["pr"] / least,
                     loca=np.where(tp > 0, c["loc_q"].astype(np.float64) / (float(SCORE_IOU_ONE) * least), np.nan))
        a["hota"] = np.sqrt(a["deta"] * a["assa"])
        out = {k: float(np.mean(v)) for k, v in a.items() if k != "loca"}
        out["loca"] = float(np.mean(a["loca"][tp > 0])) if (tp > 0).any() else float("nan")
        out["alphas"] = {k: [float(x) for x in v] for k, v in a.items()}
        out.update({k: [int(x) for x in c[k]] for k in ("tp", "fn", "fp")})
        out.update(instants=int(c["instants"]), dropped_instants=int(c["dropped_instants"]))
        return out
    names = HOTA_COUNTERS + HOTA_SUMS + ("instants", "dropped_instants")
    B = len(np.asarray(result["tp"]))
    per_lane = [{k: np.asarray(result[k])[b] for k in names} for b in range(B)]
    total = {k: sum(c[k] for c in per_lane) for k in names}
    return dict(lanes=[one(c) for c in per_lane], total=one(total))


LABEL_DEFAULTS = dict(max_keyframes=1200, max_rows=64, max_gap_us=None, min_height=None, min_diag=None)
LABEL_WORDS = ("keyframes", "head", "refused", "cut_rows", "overwritten", "labelled", "outside", "gap")
LABEL_COUNTERS = LABEL_WORDS[2:]
assert len(LABEL_WORDS) == DEFINES["DAGR_LABELS_WORDS"]
T_NEVER = int(np.iinfo(np.int64).min)                   # a lane's t_ref before its first event


def _label_options(labels, who):
    """``labels=`` of a stream, checked: None (off) or the dict of ``max_keyframes``, ``max_rows``, ``max_gap_us``,
    ``min_height`` and ``min_diag`` with the defaults filled in; refusals by name."""
    opt = _options(labels, "labels", LABEL_DEFAULTS, who)
    if opt is None:
        return None
    if not _is_int(opt["max_keyframes"]) or not 1 <= int(opt["max_keyframes"]) <= 65535:
        raise ValueError(f"{who}: labels max_keyframes = {opt['max_keyframes']!r} must be an int in 1..65535")
    if not _is_int(opt["max_rows"]) or not 1 <= int(opt["max_rows"]) <= DAGR_SCORE_MAX_GT:
        raise ValueError(f"{who}: labels max_rows = {opt['max_rows']!r} must be an int in 1..DAGR_SCORE_MAX_GT = "
                         f"{DAGR_SCORE_MAX_GT}")
    if opt["max_gap_us"] is not None and (not _is_int(opt["max_gap_us"]) or int(opt["max_gap_us"]) < 1):
        raise ValueError(f"{who}: labels max_gap_us = {opt['max_gap_us']!r} must be a positive int of microseconds (or None: "
                         "no limit)")
    for name in ("min_height", "min_diag"):
        if opt[name] is not None and not _is_real(opt[name]):
            raise ValueError(f"{who}: labels {name} = {opt[name]!r} must be a number (or None: that half of the small-box "
                             "filter is off)")
    return dict(max_keyframes=int(opt["max_keyframes"]), max_rows=int(opt["max_rows"]),
                max_gap_us=None if opt["max_gap_us"] is None else int(opt["max_gap_us"]),
                min_height=None if opt["min_height"] is None else float(opt["min_height"]),
                min_diag=None if opt["min_diag"] is None else float(opt["min_diag"]))


def labels_from_tracks(tracks):
    """One frame of a DSEC track array (fields ``t, x, y, w, h, class_id, track_id``; every row carries the frame's ``t``)
    -> ``(t int, xywh fp64 [n, 4], class_id int32 [n], track_id + 1 int64 [n])``, a keyframe as ``push`` /
    ``EventStream.push_labels`` take it.  DSEC's track ids start at 0, and the scorer and the label store reserve
    ``id <= 0`` for annotations without an identity: hence the ``+ 1``.  An empty frame has no instant and is refused."""
    if len(tracks) == 0:
        raise ValueError("labels_from_tracks: an empty frame carries no instant (push it with its t and zero rows)")
    xywh = np.stack([np.asarray(tracks[k], np.float64) for k in "xywh"], axis=1)
    return int(tracks["t"][0]), xywh, np.asarray(tracks["class_id"]).astype(np.int32), \
        np.asarray(tracks["track_id"]).astype(np.int64) + 1


class LabelDefinition:
    """The label store of the module docstring in numpy: the labelled keyframes of every lane in a ring, and the ground
    truth of a step interpolated to the step's own ``t_ref`` -- the reference's inter-frame evaluation
    (``interpolate_tracks``, then ``filter_small_bboxes``), stated per lane.  All arithmetic is fp64, all instants int64
    microseconds.  ``push(b, t, xywh, label, id)`` offers lane ``b`` one keyframe and says whether it was taken;
    ``push_arrays`` is ``dagr_stream_labels_push``'s call; ``at(t_ref)`` is ``dagr_stream_labels_at``'s.  ``counters`` is a
    dict of one int64 ``[B]`` array per name of ``LABEL_COUNTERS``; ``words()`` the lanes' words as the device state holds
    them.  The yardstick of the two kernels; nothing on the device path calls it."""

    def __init__(self, batch_size, labels=True):
        self.B = int(batch_size)
        self.options = _label_options(labels, "LabelDefinition")
        if self.options is None:
            raise ValueError("LabelDefinition: labels = None is a stream that keeps no labels")
        self.reset()

    def reset(self):
        self.frames = [[] for _ in range(self.B)]           # per lane the resident keyframes, oldest first
        self.head = np.zeros(self.B, np.int64)              # the ring index of the oldest
        self.counters = {name: np.zeros(self.B, np.int64) for name in LABEL_COUNTERS}

    def words(self):
        """int64 ``[B, DAGR_LABELS_WORDS]``, the order of ``LABEL_WORDS``."""
        return np.stack([np.array([len(f) for f in self.frames], np.int64), self.head] +
                        [self.counters[name] for name in LABEL_COUNTERS], axis=1)

    def push(self, b, t, xywh, label, id, n=None):
        """One keyframe for lane ``b``: ``n`` (default: all) rows of ``xywh`` fp64 ``[rows, 4]``, ``label``, ``id``."""
        o, c, frames = self.options, self.counters, self.frames[b]
        xywh = np.asarray(xywh, np.float64).reshape(-1, 4)
        label, id, t = np.asarray(label, np.int32).reshape(-1), np.asarray(id, np.int64).reshape(-1), int(t)
        n = len(xywh) if n is None else int(n)
        if frames and t <= frames[-1][0]:
            c["refused"][b] += 1
            return False
        kept = min(n, o["max_rows"])
        c["cut_rows"][b] += n - kept
        if len(frames) == o["max_keyframes"]:
            frames.pop(0)
            self.head[b] = (self.head[b] + 1) % o["max_keyframes"]
            c["overwritten"][b] += 1
        frames.append((t, xywh[:kept].copy(), label[:kept].copy(), id[:kept].copy()))
        return True

    def push_arrays(self, t, n, xywh, label, id):
        """``t`` int64 ``[B, F]``, ``n`` int32 ``[B, F]`` (negative: none), ``xywh`` fp64 ``[B, F, R, 4]``, ``label`` int32
        ``[B, F, R]``, ``id`` int64 ``[B, F, R]``: every lane takes its ``F`` keyframes in order."""
        t, n = np.asarray(t, np.int64), np.asarray(n, np.int32)
        for b in range(self.B):
            for f in range(t.shape[1]):
                if n[b, f] >= 0:
                    self.push(b, t[b, f], xywh[b, f], label[b, f], id[b, f], n=n[b, f])

    @staticmethod
    def _first_rows(ids):
        """The rows that take part, by ascending identity: ``id > 0``, an identity at its first row."""
        first = {}
        for g, v in enumerate(ids):
            if v > 0:
                first.setdefault(int(v), g)
        return first

    def rows_at(self, b, t):
        """Lane ``b`` at the instant ``t``, nothing counted: ``("outside" | "gap", None, None, None)`` or ``("labelled", xywh
        fp64 [m, 4], label int32 [m], id int64 [m])`` -- the surviving rows in ascending identity, before the box is made."""
        o, frames, t = self.options, self.frames[b], int(t)
        if t == T_NEVER or not frames or t < frames[0][0] or t > frames[-1][0]:
            return "outside", None, None, None
        k = max(i for i, f in enumerate(frames) if f[0] <= t)
        t0, xa, la, ia = frames[k]
        rows = self._first_rows(ia)
        if k == len(frames) - 1:                            # the newest keyframe's own instant: its rows as they are
            idents = sorted(rows)
            xywh = xa[[rows[v] for v in idents]].reshape(-1, 4)
        else:
            t1, xb, _, ib = frames[k + 1]
            if o["max_gap_us"] is not None and t1 - t0 > o["max_gap_us"]:
                return "gap", None, None, None
            partner = self._first_rows(ib)
            idents = sorted(v for v in rows if v in partner)
            a = xa[[rows[v] for v in idents]].reshape(-1, 4)
            bb = xb[[partner[v] for v in idents]].reshape(-1, 4)
            r = np.float64(t - t0) / np.float64(t1 - t0)
            with np.errstate(all="ignore"):
                xywh = a * (1 - r) + bb * r                 # two multiplies, one add
        keep = np.ones(len(idents), bool)
        with np.errstate(all="ignore"):
            w, h = xywh[:, 2], xywh[:, 3]
            if o["min_diag"] is not None:
                keep &= np.sqrt(h * h + w * w) > o["min_diag"]
            if o["min_height"] is not None:
                keep &= (w > o["min_height"]) & (h > o["min_height"])
        label = np.array([la[rows[v]] for v in idents], np.int32)
        return "labelled", xywh[keep], label[keep], np.array(idents, np.int64)[keep]

    def at(self, t_ref, out=None):
        """``t_ref`` int64 ``[B]`` -> ``(gt_box fp32 [B, G, 4] as x1 y1 x2 y2, gt_label int32 [B, G], gt_id int64 [B, G], n_gt
        int32 [B])``, ``G = max_rows``; given ``out=`` (the four arrays) it writes into them, so that what a step does not
        write stays (otherwise it is zero)."""
        G = self.options["max_rows"]
        t_ref = np.broadcast_to(np.asarray(t_ref, np.int64).reshape(-1), (self.B,))
        gt_box, gt_label, gt_id, n_gt = out if out is not None else (
            np.zeros((self.B, G, 4), np.float32), np.zeros((self.B, G), np.int32), np.zeros((self.B, G), np.int64),
            np.zeros(self.B, np.int32))
        for b in range(self.B):
            what, xywh, label, ids = self.rows_at(b, t_ref[b])
            self.counters[what][b] += 1
            if what != "labelled":
                n_gt[b] = -1
                continue
            m = len(ids)
            with np.errstate(all="ignore"):
                gt_box[b, :m, 0], gt_box[b, :m, 1] = xywh[:, 0], xywh[:, 1]
                gt_box[b, :m, 2], gt_box[b, :m, 3] = xywh[:, 0] + xywh[:, 2], xywh[:, 1] + xywh[:, 3]
            gt_label[b, :m], gt_id[b, :m], n_gt[b] = label, ids, m
        return gt_box, gt_label, gt_id, n_gt


DAGR_MAP_MAX_IMAGES = DEFINES["DAGR_MAP_MAX_IMAGES"]
DAGR_COCO_MAX_GT, DAGR_COCO_MAX_DT = DEFINES["DAGR_COCO_MAX_GT"], DEFINES["DAGR_COCO_MAX_DT"]
MAP_DEFAULTS = dict(max_images=1200, max_dets=None)
MAP_WORDS = ("images", "dropped_images", "cut_dets", "unlabelled", "empty")
assert len(MAP_WORDS) == DEFINES["DAGR_MAP_WORDS"]


def _map_options(map, who):
    """``map=`` of a stream, checked: None (off) or the dict of ``max_images`` and ``max_dets`` (None: the engine's rows per
    lane, so that nothing is cut) with the defaults filled in; refusals by name."""
    opt = _options(map, "map", MAP_DEFAULTS, who)
    if opt is None:
        return None
    if not _is_int(opt["max_images"]) or not 1 <= int(opt["max_images"]) <= DAGR_MAP_MAX_IMAGES:
        raise ValueError(f"{who}: map max_images = {opt['max_images']!r} must be an int in 1..DAGR_MAP_MAX_IMAGES = "
                         f"{DAGR_MAP_MAX_IMAGES}")
    if opt["max_dets"] is not None and (not _is_int(opt["max_dets"]) or not 1 <= int(opt["max_dets"]) <= DAGR_COCO_MAX_DT):
        raise ValueError(f"{who}: map max_dets = {opt['max_dets']!r} must be an int in 1..DAGR_COCO_MAX_DT = {DAGR_COCO_MAX_DT} "
                         "(or None: the engine's rows per lane)")
    return dict(max_images=int(opt["max_images"]), max_dets=None if opt["max_dets"] is None else int(opt["max_dets"]))


def map_det_classes(label):
    """The class a logged detection row counts for, from its fp32 label: the class whose number the label IS, -1 for a label
    that is no whole number in int32's range (it then belongs to no job) -- ``label == float(c)`` on the device.  This
    deliberately differs from the ``DetectionBuffer`` route, which truncates (``.long()``: 0.5 becomes class 0, NaN is
    undefined): the engine's detections carry whole labels, so the two agree on everything but malformed rows, and a
    rule that is defined for every fp32 value is one a kernel can equal bit for bit."""
    label = np.asarray(label, np.float32).reshape(-1)
    with np.errstate(all="ignore"):
        whole = np.isfinite(label) & (label == np.floor(label)) & (np.abs(label) < 2.0 ** 31)
    return np.where(whole, np.where(whole, label, 0).astype(np.int64), -1)


class MapDefinition:
    """The mAP log of the module docstring in numpy: which (lane, instant) becomes an image and what it keeps
    (include/dagr_hip.h, "Event stream mAP", states the rule).  ``step(det, n_keep, gt_box, gt_label, n_gt, t_ref)`` is
    ``dagr_stream_map_log``'s call; ``log[b]`` the lane's images in log order as ``(t, gt_box fp32 [g, 4], gt_label int32
    [g], det fp32 [d, 6])``; ``images()`` the protocol's lists, lane-major; ``compute()`` hands them to the host
    ``evaluate_detection``, which is the definition of the metric.  ``counters`` is a dict of one int64 ``[B]`` array per
    name of ``MAP_WORDS[1:]``; ``words()`` the lanes' words as the device state holds them.  The yardstick of the log and
    plan kernels; nothing on the device path calls it."""

    def __init__(self, batch_size, map=True):
        self.B = int(batch_size)
        self.options = _map_options(map, "MapDefinition")
        if self.options is None:
            raise ValueError("MapDefinition: map = None is a stream that keeps no mAP log")
        self.reset()

    def reset(self):
        self.log = [[] for _ in range(self.B)]
        self.counters = {name: np.zeros(self.B, np.int64) for name in MAP_WORDS[1:]}

    def words(self):
        """int64 ``[B, DAGR_MAP_WORDS]``, the order of ``MAP_WORDS``."""
        return np.stack([np.array([len(v) for v in self.log], np.int64)] + [self.counters[name] for name in MAP_WORDS[1:]], axis=1)

    def step(self, det, n_keep, gt_box, gt_label, n_gt, t_ref):
        """``det`` fp32 ``[B, A, 6]``, ``n_keep`` ``[B]``, ``gt_box`` fp32 ``[B, G, 4]``, ``gt_label`` int32 ``[B, G]``, ``n_gt``
        ``[B]`` (negative: no labels at this instant), ``t_ref`` int64 ``[B]``."""
        o, c = self.options, self.counters
        det, gt_box = np.asarray(det, np.float32), np.asarray(gt_box, np.float32)
        gt_label, t_ref = np.asarray(gt_label, np.int32), np.broadcast_to(np.asarray(t_ref, np.int64).reshape(-1), (self.B,))
        A, G = det.shape[1], gt_box.shape[1]
        for b in range(self.B):
            rows = int(n_gt[b])
            if rows <= 0:                                   # metrics only where there is a box
                c["unlabelled" if rows < 0 else "empty"][b] += 1
                continue
            if len(self.log[b]) == o["max_images"]:
                c["dropped_images"][b] += 1
                continue
            ng, nk = min(rows, G), min(max(int(n_keep[b]), 0), A)
            kept = nk if o["max_dets"] is None else min(nk, o["max_dets"])
            c["cut_dets"][b] += nk - kept
            self.log[b].append((int(t_ref[b]), gt_box[b, :ng].copy(), gt_label[b, :ng].copy(), det[b, :kept].copy()))

    def images(self):
        """``(gt, dt)``: the lists ``evaluate_detection`` takes -- one dict of ``boxes`` / ``labels`` (detections: and
        ``scores``) per image, all of lane 0's images in log order, then lane 1's, ..."""
        gt, dt = [], []
        for lane in self.log:
            for _, box, label, det in lane:
                gt.append(dict(boxes=box, labels=label.astype(np.int64)))
                dt.append(dict(boxes=det[:, :4], scores=det[:, 4], labels=map_det_classes(det[:, 5])))
        return gt, dt

    def compute(self, classes=("car", "pedestrian")):
        """``evaluate_detection`` on ``images()``, plus the lanes' words by name (int64 ``[B]`` each)."""
        from .utils.coco_eval import evaluate_detection
        out = evaluate_detection(*self.images(), classes=classes)
        out.update({name: self.words()[:, i].copy() for i, name in enumerate(MAP_WORDS)})
        return out


def frame_definition(raw, fx, fy, W, H, bgr=False):
    """The model's image of one raw sensor frame (``uint8 [H_f, W_f, 3]``), stated once: ``DSEC.preprocess_image`` plus
    ``format_data`` for a top-left crop.  Rows ``[0, fy * H)`` and columns ``[0, fx * W)`` of the frame go through
    ``_resize_area_free`` to ``W x H`` (torch's bicubic interpolation, rounded back to uint8), the channels are reversed if
    ``bgr``, and ``.float() / 255.0`` gives the result, a torch ``fp32 [3, H, W]`` on the CPU.  The yardstick of
    ``dagr_stream_frame`` (``EventStream.step(frame=...)``); nothing on the device path calls it."""
    from .data.dsec_data import _resize_area_free
    raw = np.asarray(raw)
    if raw.dtype != np.uint8 or raw.ndim != 3 or raw.shape[2] != 3:
        raise ValueError(f"frame_definition: a frame is uint8 [H_f, W_f, 3], got {raw.dtype} {raw.shape}")
    if raw.shape[0] < fy * H or raw.shape[1] < fx * W:
        raise ValueError(f"frame_definition: the frame {raw.shape[1]} x {raw.shape[0]} is smaller than the crop "
                         f"{fx * W} x {fy * H}")
    small = _resize_area_free(raw[:fy * H, :fx * W], W, H)[0]           # uint8 [3, H, W]
    if bgr:
        small = small.flip(0)
    return small.float() / 255.0


def frame_closed_form(raw, fx, fy, W, H, bgr=False):
    """``frame_definition`` in closed form, in numpy integers: what ``dagr_stream_frame`` computes.  A factor ``f`` has
    four taps per axis at ``base - 1 .. base + 2``, ``base = f * d + (f - 1) // 2``, clamped to the CROP, with the weights
    ``(-3, 19, 19, -3) / 32`` for even ``f`` and ``(0, 1, 0, 0)`` for odd ``f``; the 16-tap sum is an exact integer over
    1024, rounded half to even, clamped to ``[0, 255]`` and divided by ``255`` in fp32.  Returns ``(image fp32 [3, H, W],
    sums int64 [H, W, 3])`` -- the sums (over 1024, before rounding) let a test see which ties and overshoots a frame has."""
    raw = np.asarray(raw)

    def taps(f, n):
        base = f * np.arange(n, dtype=np.int64) + (f - 1) // 2
        idx = np.clip(base[:, None] + np.arange(-1, 3, dtype=np.int64)[None, :], 0, f * n - 1)
        return idx, np.array([-3, 19, 19, -3] if f % 2 == 0 else [0, 32, 0, 0], np.int64)
    (iy, wy), (ix, wx) = taps(fy, H), taps(fx, W)
    crop = raw[:fy * H, :fx * W].astype(np.int64)
    rows = (crop[iy] * wy[None, :, None, None]).sum(1)                  # [H, fx * W, 3]
    sums = (rows[:, ix] * wx[None, None, :, None]).sum(2)               # [H, W, 3]
    q, r = sums >> 10, sums & 1023
    q = np.clip(q + ((r > 512) | ((r == 512) & (q & 1 == 1))), 0, 255)
    if bgr:
        q = q[..., ::-1]
    return np.ascontiguousarray(q.transpose(2, 0, 1)).astype(np.float32) / np.float32(255.0), sums


class StreamDefinition:
    """The definition above in numpy: ``push`` new events, read ``window()`` / ``formatted()`` / ``counts()``.  Malformed
    pushes raise ``ValueError`` (the device path reports them in its status word instead)."""

    def __init__(self, batch_size, width, height, time_window=1000000, window_us=50000, downsample=None, sensor_size=None,
                 max_lane_events=None, denoise_us=None, refractory_us=None, flicker=None, trail_us=None):
        self.B, self.W, self.H = int(batch_size), int(width), int(height)
        self.time_window = int(time_window)
        self.window_us, self.max_lane_events = _window_and_cap(window_us, max_lane_events, time_window, batch_size,
                                                               "StreamDefinition")
        self.front = None if downsample is None else _factors(downsample, self.W, self.H, sensor_size, "StreamDefinition")
        if self.front is None and sensor_size is not None:
            raise ValueError("StreamDefinition: sensor_size is given without downsample")
        self.sensor = (self.W, self.H) if self.front is None else self.front[2:]
        self.denoise_us, self.refractory_us = _noise_options(denoise_us, refractory_us, self.B, *self.sensor,
                                                             "StreamDefinition")
        self.noise = self.denoise_us is not None or self.refractory_us is not None
        self.flicker, self.trail_us = _flicker_options(flicker, trail_us, self.B, *self.sensor, "StreamDefinition")
        self.flick = self.flicker is not None or self.trail_us is not None
        self.reset()

    def reset(self):
        self.lanes = [dict(x=np.zeros(0, np.int16), y=np.zeros(0, np.int16), t=np.zeros(0, np.int64), p=np.zeros(0, np.int8))
                      for _ in range(self.B)]
        self.t_ref = [None] * self.B
        self.t_last = [None] * self.B
        self.dropped = np.zeros(self.B, np.int64)
        self.filtered = np.zeros(self.B, np.int64)
        self.suppressed = (np.zeros(self.B, np.int64), np.zeros(self.B, np.int64))      # by the flicker / the trail stage
        if self.flick:
            self.flicker_state = flicker_state(self.B, *self.sensor)
        if self.noise:
            self.last_t = np.full((self.B, self.sensor[1], self.sensor[0]), NEVER, np.int64)
        if self.front is not None:
            fx, fy, w_in, h_in = self.front
            self.change_map = np.zeros((self.B, h_in // fy, w_in // fx), np.float32)

    def _downsample(self, x, y, t, p, batch):
        """The survivors of a checked raw push, at the cells' coordinates and cut to the model's ``W x H``."""
        fx, fy, w_in, h_in = self.front
        cells_h, cells_w = self.change_map.shape[1:]
        keep = np.zeros(len(t), bool)
        cx, cy = x.astype(np.int64) // fx, y.astype(np.int64) // fy
        for i in range(len(t)):                            # a lane's events meet their cells in arrival order
            if cx[i] >= cells_w or cy[i] >= cells_h:
                continue
            cell = (int(batch[i]), int(cy[i]), int(cx[i]))
            pol = np.float32(p[i])
            # downsample_events.py:118, change_map[y_l, x_l] += p[i] * 1.0 / (fx * fy): the float64 quotient, added to the
            # fp32 cell in float64 and rounded into it
            state = np.float32(np.float64(self.change_map[cell]) + np.float64(p[i]) * 1.0 / (fx * fy))
            if np.abs(state) >= np.float32(1):
                keep[i] = cx[i] < self.W and cy[i] < self.H
                state = np.float32(state - pol)
            self.change_map[cell] = state
        return cx[keep].astype(np.int16), cy[keep].astype(np.int16), t[keep], p[keep], batch[keep]

    def push(self, x, y, t, p, batch=None, t_now=None):
        x, y, p = np.asarray(x, np.int16), np.asarray(y, np.int16), np.asarray(p, np.int8)
        t = np.asarray(t, np.int64)
        batch = np.zeros(len(t), np.int64) if batch is None else np.asarray(batch, np.int64)
        if len(batch) and (np.any(np.diff(batch) < 0) or batch[0] < 0 or batch[-1] >= self.B):
            raise ValueError("batch is not sorted or is outside [0, batch_size)")
        if t_now is not None:
            t_now = np.broadcast_to(np.asarray(t_now, np.int64).reshape(-1), (self.B,))
        if (self.front is not None or self.noise or self.flick) and \
                np.any((x < 0) | (x >= self.sensor[0]) | (y < 0) | (y >= self.sensor[1])):
            raise ValueError("a raw event is outside the sensor")
        parts, refs = [], []
        for b in range(self.B):                           # everything is checked before anything is changed (on the RAW
            tb = t[batch == b]                            # arrays of a downsampling stream: the clock is the sensor's)
            if len(tb) and (np.any(np.diff(tb) < 0) or (self.t_last[b] is not None and tb[0] < self.t_last[b])):
                raise ValueError(f"lane {b}: a timestamp goes backwards")
            newest = int(tb[-1]) if len(tb) else self.t_last[b]
            ref = int(t_now[b]) if t_now is not None else (newest if newest is not None else self.t_ref[b])
            if ref is not None and ((newest is not None and ref < newest) or
                                    (self.t_ref[b] is not None and ref < self.t_ref[b])):
                raise ValueError(f"lane {b}: t_now is behind the lane's newest event or behind its previous t_ref")
            parts.append(newest)
            refs.append(ref)
        if self.flick:                                    # flicker / trail first: flicker would support noise below
            out = flicker_definition(self.flicker_state, x, y, t, p, batch, self.flicker, self.trail_us)
            for stage, removed in enumerate(self.suppressed, 1):
                removed += np.bincount(batch[out == stage], minlength=self.B)
            keep = out == 0
            x, y, t, p, batch = x[keep], y[keep], t[keep], p[keep], batch[keep]
        if self.noise:                                    # then the noise filter; the clock above is the unfiltered push's
            keep = denoise_definition(self.last_t, x, y, t, batch, self.denoise_us, self.refractory_us)
            self.filtered += np.bincount(batch[~keep], minlength=self.B)
            x, y, t, p, batch = x[keep], y[keep], t[keep], p[keep], batch[keep]
        if self.front is not None:
            x, y, t, p, batch = self._downsample(x, y, t, p, batch)
        for b, (newest, ref) in enumerate(zip(parts, refs)):
            m = batch == b
            lane = self.lanes[b]
            lane.update(x=np.concatenate([lane["x"], x[m]]), y=np.concatenate([lane["y"], y[m]]),
                        t=np.concatenate([lane["t"], t[m]]), p=np.concatenate([lane["p"], p[m]]))
            self.t_last[b], self.t_ref[b] = newest, ref
            if ref is not None:
                age = ref - lane["t"]
                keep = (age >= 0) & (age < self.window_us)
                for k in lane:
                    lane[k] = lane[k][keep]
            N = self.max_lane_events
            if N is not None and len(lane["t"]) > N:      # the count rule: the last N in arrival order
                self.dropped[b] += len(lane["t"]) - N
                for k in lane:
                    lane[k] = lane[k][-N:]

    def counts(self):
        return np.array([len(lane["t"]) for lane in self.lanes], np.int64)

    def window(self):
        """``(x, y, t_rel int32, p, batch int64)`` of the batch window."""
        t_rel = [(self.time_window - (self.t_ref[b] - lane["t"])).astype(np.int32) if len(lane["t"]) else
                 np.zeros(0, np.int32) for b, lane in enumerate(self.lanes)]
        cat = {k: np.concatenate([lane[k] for lane in self.lanes]) for k in ("x", "y", "p")}
        return cat["x"], cat["y"], np.concatenate(t_rel), cat["p"], np.repeat(np.arange(self.B, dtype=np.int64), self.counts())

    def formatted(self):
        """``(pos fp32[n,3], feat fp32[n,1], batch int64[n])``: the model input (``format_data``)."""
        x, y, t_rel, p, batch = self.window()
        return format_data_np(x, y, t_rel, self.W, self.H, self.time_window), p.astype(np.float32).reshape(-1, 1), batch


RENDER_DEFAULTS = dict(event_window_us=None, alpha=0.5, linewidth=1, trail=32, ids=True, id_scale=1, colors=None)
RENDER_MAX_TRAIL, RENDER_MAX_LINEWIDTH = DEFINES["DAGR_RENDER_MAX_TRAIL"], DEFINES["DAGR_RENDER_MAX_LINEWIDTH"]
RENDER_MAX_ID_SCALE = DEFINES["DAGR_RENDER_MAX_ID_SCALE"]
RENDER_STATUS_BITS = ((DEFINES["DAGR_RENDER_BAD_POLARITY"], "a drawn event's polarity p gives a channel p - 1 outside [-3, 2]"),
                      (DEFINES["DAGR_RENDER_BAD_CLASS"], "a drawn row's class has no colour"),
                      (DEFINES["DAGR_RENDER_LONG_SEGMENT"], "a trail segment is longer than W + H steps"))
RENDER_GLYPHS = tuple(ENUMS[f"DAGR_RENDER_GLYPH_{d}"] for d in range(10))      # include/dagr_hip.h holds the bitmaps
RENDER_COORD_MAX = 1 << 20
# the track palette, BGR: entry 0 is a row without a track, a track id takes 1 + (id - 1) % 31
RENDER_PALETTE = (
    (128, 128, 128), (10, 10, 216), (255, 128, 76), (12, 255, 154), (197, 65, 216), (214, 255, 12), (76, 173, 255),
    (216, 10, 62), (76, 255, 84), (93, 12, 255), (216, 160, 65), (12, 255, 235), (255, 76, 217), (113, 216, 10),
    (76, 113, 255), (255, 33, 12), (65, 216, 122), (174, 12, 255), (255, 247, 76), (10, 164, 216), (255, 76, 157),
    (52, 255, 12), (84, 65, 216), (255, 114, 12), (76, 255, 203), (216, 10, 216), (202, 255, 76), (12, 112, 255),
    (216, 65, 83), (12, 255, 54), (158, 76, 255), (216, 166, 10))


def _render_options(render, track_options, who):
    """``render=`` of a stream, checked: None (off) or the dict of ``event_window_us``, ``alpha``, ``linewidth``, ``trail``,
    ``ids``, ``id_scale`` and ``colors`` with the defaults filled in and ``colors`` resolved to a uint8 ``[n, 3]`` BGR array
    (default: ``RENDER_PALETTE`` with ``track=``, ``bbox_viz.outline_colors()`` per class without); ``track_options`` is
    what ``_track_options`` returned.  Trails and id plates are the tracker's: ``render=True`` without ``track=`` switches
    them off, a dict that asks for them without ``track=`` is refused.  Refusals by name."""
    opt = _options(render, "render", RENDER_DEFAULTS, who)
    if opt is None:
        return None
    if track_options is None:
        for key, on in (("trail", lambda v: v != 0), ("ids", lambda v: v is not False)):
            if isinstance(render, dict) and key in render and on(render[key]):
                raise ValueError(f"{who}: render {key} = {render[key]!r} needs track= (trails and id plates are the tracker's)")
        opt.update(trail=0, ids=False)
    w = opt["event_window_us"]
    if w is not None and (not _is_int(w) or not 0 <= int(w) < 1 << 63):
        raise ValueError(f"{who}: render event_window_us = {w!r} must be None (every resident event) or an int of "
                         "microseconds >= 0")
    if not _is_real(opt["alpha"]) or not 0 <= opt["alpha"] <= 1:
        raise ValueError(f"{who}: render alpha = {opt['alpha']!r} must be a float in [0, 1]")
    for key, lo, hi in (("linewidth", 1, RENDER_MAX_LINEWIDTH), ("trail", 0, RENDER_MAX_TRAIL), ("id_scale", 1, RENDER_MAX_ID_SCALE)):
        if not _is_int(opt[key]) or not lo <= int(opt[key]) <= hi:
            raise ValueError(f"{who}: render {key} = {opt[key]!r} must be an int in {lo}..{hi}")
    if not isinstance(opt["ids"], (bool, np.bool_)):
        raise ValueError(f"{who}: render ids = {opt['ids']!r} must be True or False")
    colors = opt["colors"]
    if colors is None:
        if track_options is not None:
            colors = np.array(RENDER_PALETTE, np.uint8)
        else:
            from .visualization.bbox_viz import outline_colors
            colors = outline_colors()
    else:
        colors = np.asarray(colors)
        if colors.dtype != np.uint8 or colors.ndim != 2 or colors.shape[1] != 3 or not 2 <= colors.shape[0] <= 256:
            raise ValueError(f"{who}: render colors must be a uint8 [n, 3] BGR table with 2 <= n <= 256, got "
                             f"{colors.dtype} {list(colors.shape)}")
    return dict(event_window_us=None if w is None else int(w), alpha=float(opt["alpha"]), linewidth=int(opt["linewidth"]),
                trail=int(opt["trail"]), ids=bool(opt["ids"]), id_scale=int(opt["id_scale"]),
                colors=np.ascontiguousarray(colors, dtype=np.uint8))


def render_color_index(id, n_colors):
    """The palette entry of a track id: 0 for id 0, else ``1 + (id - 1) % (n_colors - 1)``, the id as an unsigned 64-bit
    number."""
    id = int(id)
    return 0 if id == 0 else 1 + ((id - 1) % (1 << 64)) % (n_colors - 1)


def render_line(x0, y0, x1, y1):
    """The pixels of the trail segment ``(x0, y0) -> (x1, y1)``, ``k = 0 .. n`` along its major axis: int64 ``[n + 1, 2]``."""
    dx, dy = int(x1) - int(x0), int(y1) - int(y0)
    n = max(abs(dx), abs(dy))
    k = np.arange(n + 1, dtype=np.int64)
    sx, sy = (dx > 0) - (dx < 0), (dy > 0) - (dy < 0)
    if abs(dx) >= abs(dy):
        off = (2 * k * abs(dy) + n) // (2 * n) if n else 0 * k
        return np.stack([x0 + sx * k, y0 + sy * off], 1)
    off = (2 * k * abs(dx) + n) // (2 * n)
    return np.stack([x0 + sx * off, y0 + sy * k], 1)


def render_plate(id, xa, ya, scale):
    """The id plate of a row whose rectangle starts at ``(xa, ya)``: ``(left, top, mask)`` with ``mask`` a bool
    ``[7 * scale, (4 * nd + 1) * scale]`` array, True on the digits' pixels (black), False on the plate's (the row's colour)."""
    text = str((int(id) % (1 << 64)) % 1000000)
    s, nd = int(scale), len(text)
    cells = np.zeros((7, 4 * nd + 1), bool)
    for d, ch in enumerate(text):
        bits = RENDER_GLYPHS[int(ch)]
        for gy in range(5):
            for gx in range(3):
                cells[1 + gy, 1 + 4 * d + gx] = (bits >> (14 - (gy * 3 + gx))) & 1
    top = ya - 7 * s if ya - 7 * s >= 0 else ya + 1
    return int(xa), int(top), np.repeat(np.repeat(cells, s, 0), s, 1)


def _render_coord(v):
    """``(int32)floorf(clamp(v, -2^20, 2^20))`` of finite fp32 values."""
    return np.floor(np.clip(np.asarray(v, np.float32), -RENDER_COORD_MAX, RENDER_COORD_MAX)).astype(np.int64)


class RenderDefinition:
    """The picture of include/dagr_hip.h (``dagr_stream_trail`` / ``dagr_stream_render``) in numpy.  ``trail_step`` is one
    ``dagr_stream_trail`` on the tracker's slots (what ``TrackDefinition`` or ``EventStream.tracks`` hold: ``id``,
    ``t_last``, ``box`` over ``[B, max_tracks]``) and keeps the rings (``ring_id``, ``ring_count``, ``ring_pt``);
    ``frames`` paints the lanes' frames from the resident events (``lanes`` / ``t_ref`` as ``StreamDefinition`` keeps them,
    fed the stream's pushes), the step's ``det`` / ``n_keep`` and ``track_id``, and returns uint8 ``[B, H, W, 3]``;
    ``status`` accumulates the flags.  ``render`` as ``EventStream`` takes it; ``max_tracks`` None: no tracker."""

    def __init__(self, batch_size, width, height, render=True, max_tracks=None):
        self.B, self.W, self.H = int(batch_size), int(width), int(height)
        self.M = None if max_tracks is None else int(max_tracks)
        self.options = _render_options(render, None if max_tracks is None else True, "RenderDefinition")
        if self.options is None:
            raise ValueError("RenderDefinition: render = None draws nothing")
        self.reset()

    def reset(self):
        T = self.options["trail"]
        self.status = 0
        self.ring_id = self.ring_count = self.ring_pt = None
        if T > 0:
            self.ring_id = np.zeros((self.B, self.M), np.int64)
            self.ring_count = np.zeros((self.B, self.M), np.int32)
            self.ring_pt = np.zeros((self.B, self.M, T, 2), np.int32)

    def trail_step(self, slot_id, slot_t_last, slot_box, t_ref):
        """One ``dagr_stream_trail``: ``slot_id`` / ``slot_t_last`` int64 ``[B, M]``, ``slot_box`` fp32 ``[B, M, 4]`` as the
        tracker left them, ``t_ref`` the step's instants (``None`` or ``NEVER``: the lane has none)."""
        T = self.options["trail"]
        if T == 0:
            return
        box = np.asarray(slot_box, np.float32).reshape(self.B, self.M, 4)
        for b in range(self.B):
            ref = NEVER if t_ref[b] is None else int(t_ref[b])
            for s in range(self.M):
                id = int(slot_id[b][s])
                if id == 0:                             # a free slot
                    self.ring_id[b, s], self.ring_count[b, s] = 0, 0
                    continue
                if int(self.ring_id[b, s]) != id:       # the slot has been taken by another track
                    self.ring_id[b, s], self.ring_count[b, s] = id, 0
                if ref == NEVER or int(slot_t_last[b][s]) != ref:
                    continue                            # not seen this step: a coasting track appends nothing
                with np.errstate(over="ignore", invalid="ignore"):
                    cx = np.float32(box[b, s, 0] + box[b, s, 2]) * np.float32(0.5)
                    cy = np.float32(box[b, s, 1] + box[b, s, 3]) * np.float32(0.5)
                if not (np.isfinite(cx) and np.isfinite(cy)):
                    continue
                c = int(self.ring_count[b, s])
                self.ring_pt[b, s, c % T] = (_render_coord(cx), _render_coord(cy))
                c += 1
                self.ring_count[b, s] = T + (1 << 30) % T if c >= 1 << 30 else c

    def ring_points(self, b, s):
        """The points of ring ``(b, s)``, oldest first: int32 ``[n, 2]``."""
        T, c = self.options["trail"], int(self.ring_count[b, s])
        if c <= T:
            return self.ring_pt[b, s, :c]
        return self.ring_pt[b, s, (c + np.arange(T)) % T]

    def events_layer(self, img, x, y, p):
        """Layer 2 on one lane's image (uint8 ``[H, W, 3]``, in place): the in-window events ``x``, ``y``, ``p`` in arrival
        order, by ``draw_events_on_image``'s rule."""
        alpha = np.float64(self.options["alpha"])
        last = {}
        for i in range(len(x)):
            ch = int(p[i]) - 1
            if ch < -3 or ch > 2:
                self.status |= RENDER_STATUS_BITS[0][0]
                continue
            if 0 <= int(x[i]) < self.W and 0 <= int(y[i]) < self.H:
                last[(int(y[i]), int(x[i]))] = ch
        for (yy, xx), ch in last.items():
            v = np.trunc(alpha * img[yy, xx].astype(np.float64)).astype(np.uint8)
            v[ch] = np.uint8(int(np.trunc(np.float64(v[ch]) + 255.0 * (1.0 - alpha))) & 255)
            img[yy, xx] = v

    def frames(self, lanes=None, t_ref=None, det=None, n_keep=None, track_id=None, base=None):
        """The frames of a step.  ``lanes``: per lane a dict of ``x``, ``y``, ``t``, ``p`` (the resident events in arrival
        order; None: no events), ``t_ref`` per lane (None / ``NEVER``: none yet); ``det`` fp32 ``[B, A, 6]``, ``n_keep``
        ``[B]`` (None: no rows); ``track_id`` int64 ``[B, A]`` or None (colour by class); ``base`` uint8 ``[B, H, W, 3]`` or
        ``[H, W, 3]`` or None (black)."""
        o, B, H, W = self.options, self.B, self.H, self.W
        colors, hw, s = o["colors"], o["linewidth"] // 2, o["id_scale"]
        n_colors = len(colors)
        out = np.zeros((B, H, W, 3), np.uint8)
        if base is not None:
            out[:] = np.asarray(base, np.uint8)
        for b in range(B):
            img = out[b]
            ref = None if lanes is None or t_ref is None or t_ref[b] is None or int(t_ref[b]) == NEVER else int(t_ref[b])
            if ref is not None:                                                             # 2 events
                lane = lanes[b]
                t = np.asarray(lane["t"], np.int64)
                keep = np.ones(len(t), bool)
                if o["event_window_us"] is not None:
                    keep = np.array([0 <= ref - int(v) < o["event_window_us"] for v in t], bool)
                self.events_layer(img, np.asarray(lane["x"])[keep], np.asarray(lane["y"])[keep], np.asarray(lane["p"])[keep])
            if self.ring_id is not None:                                                    # 3 trails: a higher slot on top
                for slot in range(self.M):
                    pts = self.ring_points(b, slot).astype(np.int64)
                    if int(self.ring_id[b, slot]) == 0 or len(pts) < 2:
                        continue
                    c = colors[render_color_index(self.ring_id[b, slot], n_colors)]
                    for p0, p1 in zip(pts[:-1], pts[1:]):
                        if max(abs(int(p1[0] - p0[0])), abs(int(p1[1] - p0[1]))) > W + H:
                            self.status |= RENDER_STATUS_BITS[2][0]
                            continue
                        q = render_line(p0[0], p0[1], p1[0], p1[1])
                        q = q[(q[:, 0] >= 0) & (q[:, 0] < W) & (q[:, 1] >= 0) & (q[:, 1] < H)]
                        img[q[:, 1], q[:, 0]] = c
            if det is None:
                continue
            A = int(np.asarray(det).shape[1])
            rows = []
            for r in range(min(max(int(n_keep[b]), 0), A)):                                  # 4 boxes, a later row on top
                d = np.asarray(det[b][r], np.float32)
                if not np.all(np.isfinite(d[:4])):
                    continue
                cx1, cy1, cx2, cy2 = (int(v) for v in _render_coord(d[:4]))
                xa, xb, ya, yb = min(cx1, cx2), max(cx1, cx2), min(cy1, cy2), max(cy1, cy2)
                if track_id is not None:
                    id = int(track_id[b][r])
                    c = colors[render_color_index(id, n_colors)]
                else:
                    id = 0
                    if not 0 <= d[5] < n_colors:
                        self.status |= RENDER_STATUS_BITS[1][0]
                        continue
                    c = colors[int(d[5])]
                x_lo, x_hi, y_lo, y_hi = max(xa - hw, 0), min(xb + hw, W - 1), max(ya - hw, 0), min(yb + hw, H - 1)
                if x_lo <= x_hi and y_lo <= y_hi:           # (the band lies inside this window of the image)
                    yy, xx = np.mgrid[y_lo:y_hi + 1, x_lo:x_hi + 1]
                    inside = (xx >= xa) & (xx <= xb) & (yy >= ya) & (yy <= yb)
                    dist = np.where(inside, np.minimum(np.minimum(xx - xa, xb - xx), np.minimum(yy - ya, yb - yy)),
                                    np.maximum(np.maximum(np.maximum(xa - xx, xx - xb), 0),
                                               np.maximum(np.maximum(ya - yy, yy - yb), 0)))
                    img[y_lo:y_hi + 1, x_lo:x_hi + 1][dist <= hw] = c
                rows.append((id, xa, ya, c))
            for id, xa, ya, c in rows if o["ids"] else ():                                  # 5 plates, above every outline
                if id == 0:
                    continue
                left, top, mask = render_plate(id, xa, ya, s)
                x_lo, x_hi, y_lo, y_hi = max(left, 0), min(left + mask.shape[1], W), max(top, 0), min(top + mask.shape[0], H)
                if x_lo < x_hi and y_lo < y_hi:             # clipped to the image per pixel
                    part = mask[y_lo - top:y_hi - top, x_lo - left:x_hi - left]
                    img[y_lo:y_hi, x_lo:x_hi] = np.where(part[:, :, None], np.uint8(0), c)
        return out


DECODE_FORMATS = {"evt2": (DEFINES["DAGR_DECODE_EVT2"], np.uint32, 1), "evt3": (DEFINES["DAGR_DECODE_EVT3"], np.uint16, 12)}
DECODE_COUNTERS = ("decoded", "unsynced", "outside", "skipped")
DECODE_STATE = ("high", "low", "loops", "y", "base_x", "pol", "synced")


def _decode_options(decode, max_decoded, sensor_w, sensor_h, who):
    """``(format name, max_decoded or None)`` of a decoding stream over a ``sensor_w x sensor_h`` sensor, checked; refusals
    by name."""
    if decode not in DECODE_FORMATS:
        raise ValueError(f"{who}: decode = {decode!r} must be None (off), 'evt2' or 'evt3'")
    if max_decoded is not None and (not _is_int(max_decoded) or not 1 <= int(max_decoded) < 1 << 30):
        raise ValueError(f"{who}: max_decoded = {max_decoded!r} must be an int in 1..2**30 - 1 (or None: the worst case of "
                         "every push)")
    if not (1 <= int(sensor_w) <= 32767 and 1 <= int(sensor_h) <= 32767):
        raise ValueError(f"{who}: the sensor {sensor_w} x {sensor_h} does not fit the int16 pixel coordinates (1..32767 per "
                         "axis)")
    return decode, None if max_decoded is None else int(max_decoded)


def _decode_t_base(t_base, batch_size, who):
    """``t_base`` of a decoding stream as int64 ``[B]`` (None: zeros; a scalar serves every lane)."""
    if t_base is None:
        return np.zeros(int(batch_size), np.int64)
    a = np.asarray(t_base)
    if a.dtype.kind not in "iu" or a.size not in (1, int(batch_size)):
        raise ValueError(f"{who}: t_base = {t_base!r} must be an int or one int per lane ({int(batch_size)})")
    return np.array(np.broadcast_to(a.astype(np.int64).reshape(-1), (int(batch_size),)))


def words_as_array(words, decode, who):
    """The words of a push as a contiguous array of the format's word type: ``words`` is such an array, or ``bytes`` / a
    uint8 array whose length is a multiple of the word size (little-endian)."""
    dtype = np.dtype(DECODE_FORMATS[decode][1])
    if isinstance(words, (bytes, bytearray, memoryview)):
        words = np.frombuffer(words, np.uint8)
    words = np.ascontiguousarray(np.asarray(words)).reshape(-1)
    if words.dtype == np.uint8:
        if words.size % dtype.itemsize:
            raise ValueError(f"{who}: {words.size} bytes are not a whole number of {dtype.itemsize}-byte {decode} words")
        return words.view(dtype.newbyteorder("<")).astype(dtype, copy=False)
    if words.dtype != dtype:
        raise ValueError(f"{who}: {decode} words are {dtype.name} (or bytes / uint8), got {words.dtype.name}")
    return words


def _lane_words(lane_words, n_words, batch_size, who):
    """``lane_words`` of a push as int64 ``[B]``: words per lane, in lane order (default: all to lane 0 when ``B == 1``)."""
    if lane_words is None:
        if int(batch_size) != 1:
            raise ValueError(f"{who}: lane_words is required with {int(batch_size)} lanes (words per lane, in lane order)")
        return np.array([n_words], np.int64)
    a = np.asarray(lane_words)
    if a.dtype.kind not in "iu" or a.shape != (int(batch_size),) or (a.astype(np.int64) < 0).any() or int(a.sum()) != n_words:
        raise ValueError(f"{who}: lane_words = {lane_words!r} must be {int(batch_size)} non-negative ints that sum to the "
                         f"number of words ({n_words})")
    return a.astype(np.int64)


class DecodeDefinition:
    """The decoder of the module docstring as the sequential loop it is stated as: ``push(words, lane_words)`` decodes one
    push of every lane and returns ``(x int16, y int16, t int64, p int8, batch int32)``, at most ``max_out`` rows (None:
    all).  ``counts`` is the dict of the four int64 ``[B]`` counters, ``state`` the dict of the lanes' states (int64 ``[B]``
    each), ``status`` the bits the pushes have raised (16: outside the sensor, 64: more than ``max_out``).  The yardstick of
    ``dagr_stream_decode``; nothing on the device path calls it."""

    def __init__(self, batch_size, format, sensor_w, sensor_h, t_base=None, max_out=None):
        self.B = int(batch_size)
        self.format, self.max_out = _decode_options(format, max_out, sensor_w, sensor_h, "DecodeDefinition")
        self.sensor_w, self.sensor_h = int(sensor_w), int(sensor_h)
        self.t_base = _decode_t_base(t_base, self.B, "DecodeDefinition")
        self.reset()

    def reset(self):
        self.state = {k: np.zeros(self.B, np.int64) for k in DECODE_STATE}
        self.counts = {k: np.zeros(self.B, np.int64) for k in DECODE_COUNTERS}
        self.status = 0

    def push(self, words, lane_words=None):
        words = words_as_array(words, self.format, "DecodeDefinition")
        lane_words = _lane_words(lane_words, len(words), self.B, "DecodeDefinition")
        evt3 = self.format == "evt3"
        out, at = [], 0
        for b in range(self.B):
            s = {k: int(v[b]) for k, v in self.state.items()}
            c = {k: 0 for k in DECODE_COUNTERS}
            t0 = int(self.t_base[b])

            def emit(x, y, pol, low, shift_high, shift_loops):
                if not s["synced"]:
                    c["unsynced"] += 1
                elif not (x < self.sensor_w and y < self.sensor_h):
                    c["outside"] += 1
                    self.status |= 16
                else:
                    c["decoded"] += 1
                    out.append((x, y, t0 + (s["loops"] << shift_loops) + (s["high"] << shift_high) + low, 1 if pol else -1, b))

            def time_high(v, wrap):
                if s["synced"] and s["high"] - v >= wrap:
                    s["loops"] += 1
                s["high"], s["synced"] = v, 1

            for w in words[at:at + int(lane_words[b])].tolist():
                if evt3:
                    kind = w >> 12
                    if kind == 0x0:
                        s["y"] = w & 0x7FF
                    elif kind == 0x2:
                        emit(w & 0x7FF, s["y"], (w >> 11) & 1, s["low"], 12, 24)
                    elif kind == 0x3:
                        s["base_x"], s["pol"] = w & 0x7FF, (w >> 11) & 1
                    elif kind in (0x4, 0x5):
                        bits = 12 if kind == 0x4 else 8
                        for i in range(bits):
                            if (w >> i) & 1:
                                emit((s["base_x"] + i) & 0xFFFFFFFF, s["y"], s["pol"], s["low"], 12, 24)
                        s["base_x"] = (s["base_x"] + bits) & 0xFFFFFFFF
                    elif kind == 0x6:
                        s["low"] = w & 0xFFF
                    elif kind == 0x8:
                        time_high(w & 0xFFF, 2048)
                    else:
                        c["skipped"] += 1
                else:
                    kind = w >> 28
                    if kind <= 1:
                        emit((w >> 11) & 0x7FF, w & 0x7FF, kind, (w >> 22) & 0x3F, 6, 34)
                    elif kind == 0x8:
                        time_high(w & 0x0FFFFFFF, 1 << 27)
                    else:
                        c["skipped"] += 1
            at += int(lane_words[b])
            for k in DECODE_STATE:
                self.state[k][b] = s[k]
            for k in DECODE_COUNTERS:
                self.counts[k][b] += c[k]
        if self.max_out is not None and len(out) > self.max_out:
            self.status |= 64
            out = out[:self.max_out]
        cols = list(zip(*out)) if out else [[]] * 5
        return (np.array(cols[0], np.int16), np.array(cols[1], np.int16), np.array(cols[2], np.int64),
                np.array(cols[3], np.int8), np.array(cols[4], np.int32))


def _flag_names(flag):
    return "; ".join(text for bit, text in STATUS_BITS if flag & bit)


class EventStream:
    """Detections every step from an endless event stream, on the last ``window_us`` microseconds of every lane --
    with ``max_lane_events=N`` on the newest ``N`` events of them at most (``window_us=None``: on the newest ``N`` events of
    the model's time window).  A capped stream has the constant capacity ``B * N``: after its first step no buffer grows
    and no graph is captured again, however many ``step_device`` calls follow without a read-back, and a burst costs its
    own lane's oldest events only; ``dropped()`` counts them.  (A downsampling stream's front still sizes its scratch by
    the largest raw push.)

    ``model``: an eval-mode ``DAGR`` on the GPU whose window engine runs the captured window: the tiled level-0 conv
    (``l0_tiles``), the event path (no ``--no_events``), the engine path (``model.module_path_only`` False).
    ``downsample`` (``f`` or ``(fx, fy)``) and ``sensor_size`` (``(W_in, H_in)``, default ``(fx * W, fy * H)``): the
    pushes carry raw sensor events, which ``dagr_stream_downsample`` turns into the model's on the device (module
    docstring); ``change_maps()`` reads the integrators back.
    ``denoise_us`` and ``refractory_us`` (positive ints of microseconds, ``None``: off): ``dagr_stream_denoise`` removes
    background activity and hot pixels from every push on the device, before anything else (module docstring);
    ``filtered()`` counts what it removed, ``last_stamps()`` reads the stamp maps back.  A stream built without them issues
    exactly the launches it issues without the filter.
    ``flicker`` (``None``: off, ``True``: the defaults, or a dict of ints ``min_hz``, ``max_hz``, ``start``, ``stop``,
    ``max_count``) and ``trail_us`` (a positive int of microseconds, ``None``: off): ``dagr_stream_flicker`` removes the
    events of pixels that flicker at a steady rate between ``min_hz`` and ``max_hz``, and the same-polarity events that
    trail another by less than ``trail_us``, from every push on the device -- behind the decoder, in front of the noise
    filter (module docstring: this project's statement of two well-known filters, not a vendor's algorithm; the defaults
    are conventions, not measured optima; tested on synthetic flicker only).  ``suppressed()`` counts what either stage
    removed, ``flicker_state()`` reads the per-pixel state back.  A stream built without them makes exactly the library
    calls it makes without the filter.
    ``track`` (``None``: off, ``True``: the defaults, or a dict of ``iou``, ``max_age_us``, ``min_score``, ``max_tracks``):
    every step ends with ``dagr_stream_track``, one more launch and no host wait, which gives every detection the id of
    the track it continues (module docstring).  ``track_ids`` / ``track_hits`` are the step's device tensors, ``step()``
    adds ``"track_ids"`` / ``"track_hits"`` to every lane's dict, ``tracks()`` reads the live tracks back and
    ``untracked()`` counts the rows that got no id.  A stream built without it issues exactly the launches it issues
    without the tracker.
    ``motion`` (``None``: off, ``True``: the defaults, or a dict of ``alpha``, ``beta``; needs ``track``): the tracker
    carries a velocity per track and matches against predicted boxes (module docstring), so a track survives a gap; the
    step's one tracker launch is then ``dagr_stream_track_cv``.  ``track_boxes`` / ``track_vel`` are the step's filtered
    boxes and velocities per detection row, ``step()`` adds ``"track_boxes"`` / ``"track_vel"``, ``coasting()`` reads back
    the tracks the step did not see with their predicted boxes (``coast_device()``: the device tensors), and ``tracks()``
    appends the velocities.  A stream built without it issues exactly the calls it issues without the motion model.
    ``rescue`` (``None``: off, ``True``: the defaults, or a dict of ``low_score``, ``iou``; needs ``track`` with a
    ``min_score`` above ``low_score``): a second association round in the same launch lets the rows under ``min_score``
    continue tracks that no confident row matched, and never start one (module docstring); the step's one tracker launch
    is then ``dagr_stream_track_rescue`` or ``dagr_stream_track_cv_rescue``.  ``rescued()`` counts its matches.  The
    defaults are ByteTrack's conventions, not measured optima.  A stream built without it issues exactly the calls it
    issues without the round.
    ``assign`` (``None`` or ``"greedy"``: the greedy match; ``"optimal"``; needs ``track``): the match of every round is an
    optimal one-to-one assignment -- the most matches, then the largest sum of IoUs quantised to 2**-20 (module docstring)
    -- with ``motion`` and ``rescue`` composing as they do without it; the step's one tracker launch is then
    ``dagr_stream_track_optimal``, on the same state, with a workspace the stream owns.  A stream built without it issues
    exactly the calls it issues without it.
    ``score`` (``None``: off, ``True``: the defaults, or a dict of ``iou``, ``max_objects``, ``boxes``; needs ``track``):
    ``score_step(gt_box, gt_label, gt_id, n_gt)`` scores the last step's track ids against labelled boxes on the device --
    this project's statement of the CLEAR-MOT counts with a greedy matcher (module docstring) --, ``track_score()`` reads
    the counters back, ``scored_objects()`` the object tables, and ``score_summary`` turns both into MOTA, MOTP and the id
    switches.  A step of a scoring stream issues exactly the calls it issues without the scorer: only ``score_step``
    launches (``dagr_stream_score``, once).  A stream built without it issues exactly the calls it issued before.
    ``identity`` (``None``: off, ``True``: the default, or ``dict(max_tracks=N)``; needs ``score``): ``score_step`` issues
    ``dagr_stream_identity`` behind ``dagr_stream_score`` -- two launches, still no host wait -- and ``identity()`` runs the
    maximum-weight assignment on the counts (``dagr_stream_identity_solve``) and returns IDF1's integers (module docstring;
    ``identity_summary`` gives IDF1, IDP and IDR); ``identity_tables()`` reads the state back.  A stream built without it
    issues exactly the calls it issued before.
    ``hota`` (``None``: off, ``True``: the default, or ``dict(max_instants=N)``, 1 .. ``DAGR_HOTA_MAX_INSTANTS``, default
    1200; needs ``identity``): ``score_step`` issues ``dagr_stream_hota`` behind ``dagr_stream_identity`` -- three launches,
    still no host wait --, which runs HOTA's pass 1 and appends the labelled instant to the lane's log on the device;
    ``hota()`` replays the log (``dagr_stream_hota_solve``: one optimal assignment per logged instant, 19 thresholds) and
    returns HOTA's integers and fp64 sums (module docstring; ``hota_summary`` gives HOTA, DetA, AssA and LocA);
    ``hota_tables()`` reads the state back.  A combination whose state would exceed ``DAGR_HOTA_MAX_STATE_BYTES`` is
    refused by name.  A stream built without it issues exactly the calls it issued before.
    ``labels`` (``None``: off, ``True``: the defaults, or a dict of ``max_keyframes``, ``max_rows``, ``max_gap_us``,
    ``min_height``, ``min_diag``; needs neither ``track`` nor ``score``): the stream keeps labelled keyframes
    (``push_labels``) and interpolates the ground truth to the last step's own ``t_ref`` on the device (module docstring):
    ``labels_step()`` is the one launch (``dagr_stream_labels_at``), ``score_step()`` without arguments runs it in front
    of the scorer chain, ``label_counts()`` reads the counters back.  A step of such a stream issues exactly the calls it
    issues without the store, and a stream built without it issues exactly the calls it issued before.
    ``map`` (``None``: off, ``True``: the defaults, or a dict of ``max_images`` -- 1 .. ``DAGR_MAP_MAX_IMAGES``, default 1200
    a lane -- and ``max_dets`` -- ``None``: the engine's rows per lane, so that nothing is cut; needs neither ``track`` nor
    ``score``): detection mAP over every step.  ``map_step()`` appends the last step's detections and its ground truth --
    the interpolated keyframes of a ``labels=`` stream, or the caller's tensors -- to a log of fixed capacity on the device
    (``dagr_stream_map_log``: one launch, no host wait; only lanes with at least one box are logged, as
    ``evaluated_images`` has it), and ``map()`` builds the COCO protocol's job list from the log on the device
    (``dagr_stream_map_plan``), runs ``dagr_coco_match`` and ``dagr_coco_accumulate`` on it and returns what
    ``evaluate_detection`` returns, with the log's counters (include/dagr_hip.h states the rule, ``MapDefinition`` is the
    same in numpy and hands its images to the host ``evaluate_detection``, the definition of the metric).  ``map_counts()``
    / ``map_log()`` read the counters and the log back.  Memory: the log (first ``map_step()``) and the plan's arrays (first
    ``map()``) are sized from the capacities and allocated once, about ``64 * B * max_images * max_dets`` bytes together --
    2.6 GB at B = 8 with the defaults on an engine of 4096 rows a lane; a trained model keeps few rows, so
    ``map=dict(max_dets=100)`` (the protocol evaluates 100 a class and image at most) brings that under 100 MB.  A step of such a stream issues exactly the calls it issues
    without the log, and a stream built without it issues exactly the calls it issued before.
    ``decode`` (``None``: off, ``"evt2"`` or ``"evt3"``), ``max_decoded`` and ``t_base``: the stream takes the camera's words
    (``step_words`` / ``step_words_device``) and ``dagr_stream_decode`` turns them into events on the device, in front of
    the filter, the front and the window (module docstring; the formats as recalled from the vendor's public descriptions,
    not confirmed against a camera file).  The sensor is ``(W, H)``, or ``sensor_size`` with ``downsample=``.
    ``max_decoded=None`` sizes the decoded events' buffers for the worst case of every push, so that status bit 6 cannot
    occur; a smaller int makes the fronts behind the decoder cheaper and may raise it.  ``t_base`` (an int or one per lane)
    is added to every decoded timestamp.  ``decode_counts()`` / ``decode_state()`` read the counters and the lanes' states
    back.  The host's bound of the window grows by the worst case of every push, so a decoding stream that is never read
    back should be capped (``max_lane_events``).  A stream built without ``decode`` makes exactly the calls it makes
    without the decoder.
    ``frame_size`` (``(W_f, H_f)``) and ``frame_bgr``: the steps may carry raw sensor frames (``frame=``), which
    ``dagr_stream_frame`` turns into the model's image on the device (``frame_definition``) with the stream's
    ``downsample`` factors, or 1 without ``downsample``.
    ``render`` (``None``: off, ``True``: the defaults, or a dict of ``event_window_us``, ``alpha``, ``linewidth``, ``trail``,
    ``ids``, ``id_scale``, ``colors``): ``render_step(base=None, out=None)`` paints the lanes' frames on the device --
    the resident events of the last ``event_window_us`` microseconds (``None``: all of them), the trails of the last
    ``trail`` centres of every track, the step's box outlines in the colour of their track id (without ``track=``: of
    their class) and the ids on plates -- from the stream's own arrays: ``dagr_stream_render``, three launches at most, no
    host wait, nothing uploaded (include/dagr_hip.h states the rule, ``RenderDefinition`` is the same in numpy; the look is
    this project's own).  The frames are the engine's ``H x W`` -- with ``downsample=`` the model's resolution, where the
    resident events live.  Trails and plates need ``track=``: ``render=True`` without it draws neither, a dict that asks
    for one is refused.  A step of a tracking stream with ``trail > 0`` issues one more launch right behind the
    tracker's, ``dagr_stream_trail``; nothing else in a step changes, and a stream built without ``render`` issues exactly
    the calls it issued before.  ``trails()`` reads the rings back, ``render_status()`` the picture's flags.

    ``--use_image`` models: the image branch runs once per frame.  A step runs the frame body (image branch included)
    when it brings a frame (``image=`` or ``frame=``; contents are not compared), on the stream's first step, and whenever
    something has rewritten the memory the frame's maps live in since the stream's last frame body -- any other window on
    the same engine (a plain ``model(...)`` / ``forward_detections`` call, another stream), a buffer that grew, a change of
    thresholds or of the frame's shape, a switch between latency and throughput mode.  Every other step runs the held
    body, which samples the maps the last frame body left.  The engine tracks this itself; ``frame_steps`` /
    ``held_steps`` count the bodies run, and the result is what ``reset=True`` gives with the frame in force either way.
    """

    def __init__(self, model, window_us=50000, downsample=None, sensor_size=None, frame_size=None, frame_bgr=False,
                 max_lane_events=None, denoise_us=None, refractory_us=None, track=None, motion=None, rescue=None,
                 decode=None, max_decoded=None, t_base=None, flicker=None, trail_us=None, score=None,
                 identity=None, assign=None, hota=None, labels=None, render=None, map=None):
        import torch
        self.model = model
        self.labels = _label_options(labels, "EventStream")
        self.map_options = _map_options(map, "EventStream")
        self.track = _track_options(track, "EventStream")
        self.render = _render_options(render, self.track, "EventStream")
        self.motion = _motion_options(motion, self.track, "EventStream")
        self.rescue = _rescue_options(rescue, self.track, "EventStream")
        self.assign = _assign_options(assign, self.track, "EventStream")
        self.score = _score_options(score, self.track, self.motion, "EventStream")
        self.identity_options = _identity_options(identity, self.score, "EventStream")
        self.hota_options = _hota_options(hota, self.identity_options, "EventStream")
        time_window = int(getattr(model.args, "time_window_us", 1000000))
        self.window_us, self.max_lane_events = _window_and_cap(window_us, max_lane_events, time_window,
                                                               getattr(model.args, "batch_size", 1), "EventStream")
        if model.training:
            raise RuntimeError("EventStream needs an eval-mode model (model.eval())")
        dev = next(model.parameters()).device
        if dev.type != "cuda" or not torch.cuda.is_available():
            raise RuntimeError(f"EventStream needs the model on the GPU (it is on {dev}): the stream lives in device "
                               "memory and there is no CPU path")
        if model.module_path_only:
            raise RuntimeError("EventStream: module_path_only is set (--keep_temporal_ordering models run module by module); "
                               "set model.module_path_only = False to run the window engine")
        if bool(getattr(model.args, "no_events", False)):
            raise RuntimeError("EventStream: --no_events returns the image branch's detections; there is no event window to slide")
        eng = model.engine()
        if not eng.l0_tiles:
            raise RuntimeError("EventStream: l0_tiles is off for this model (the captured window needs the tiled level-0 "
                               "conv: a 3x3 / 3x5 / 5x3 tap window and max_neighbors = 16)")
        from .engine import StreamState
        self.device = dev
        self.B = eng.B
        if self.max_lane_events is not None:
            _window_and_cap(self.window_us, self.max_lane_events, time_window, eng.B, "EventStream")
        self.state = StreamState(eng.B, self.window_us, dev, max_lane_events=self.max_lane_events)
        w_in, h_in = eng.W, eng.H
        if downsample is not None:
            fx, fy, w_in, h_in = _factors(downsample, eng.W, eng.H, sensor_size, "EventStream")
        elif sensor_size is not None:
            raise ValueError("EventStream: sensor_size is given without downsample")
        self.denoise_us, self.refractory_us = _noise_options(denoise_us, refractory_us, eng.B, w_in, h_in, "EventStream")
        self.flicker, self.trail_us = _flicker_options(flicker, trail_us, eng.B, w_in, h_in, "EventStream")
        self.decode, self.max_decoded = None, None
        if decode is not None:
            self.decode, self.max_decoded = _decode_options(decode, max_decoded, w_in, h_in, "EventStream")
            self.t_base = _decode_t_base(t_base, eng.B, "EventStream")
            self.state.enable_decode(DECODE_FORMATS[self.decode][0], w_in, h_in, self.max_decoded,
                                     self.t_base if self.t_base.any() else None)
        elif max_decoded is not None or t_base is not None:
            raise ValueError("EventStream: max_decoded / t_base are given without decode")
        if downsample is not None:
            self.state.enable_front(fx, fy, w_in, h_in, eng.W, eng.H)
        if self.denoise_us is not None or self.refractory_us is not None:
            self.state.enable_denoise(w_in, h_in, self.denoise_us, self.refractory_us)
        if self.flicker is not None or self.trail_us is not None:
            self.state.enable_flicker(w_in, h_in, self.flicker, self.trail_us)
        if self.track is not None:
            self.state.enable_track(self.track, motion=self.motion, rescue=self.rescue, assign=self.assign)
        if self.score is not None:
            self.state.enable_score(self.score)
        if self.identity_options is not None:
            self.state.enable_identity(self.identity_options)
        if self.hota_options is not None:
            self.state.enable_hota(self.hota_options)
        if self.labels is not None:
            self.state.enable_labels(self.labels)
        if self.map_options is not None:
            rows = sum(int(h) * int(w) for h, w in eng.out_sizes)
            if rows > DAGR_COCO_MAX_DT:
                raise ValueError(f"EventStream: map = the engine has {rows} detection rows per lane, the log takes at most "
                                 f"DAGR_COCO_MAX_DT = {DAGR_COCO_MAX_DT}")
            self.state.enable_map(self.map_options, eng.num_classes)
        if self.render is not None:
            self.state.enable_render(self.render, eng.W, eng.H)
        self._label_newest = [None] * eng.B     # per lane the newest instant a HOST push has offered (push_labels' check)
        self._zeros = None
        self.outputs = None      # the last step's decoded head outputs [B, A, 5 + classes], valid until the engine's next call
        self._frame = None
        if frame_size is not None:
            fx, fy = self.state.front[:2] if self.state.front is not None else (1, 1)
            w_f, h_f = int(frame_size[0]), int(frame_size[1])
            if w_f < fx * eng.W or h_f < fy * eng.H:
                raise ValueError(f"EventStream: frame_size {w_f} x {h_f} is smaller than the crop {fx * eng.W} x {fy * eng.H} "
                                 f"(downsample {fx} x {fy} over the model's {eng.W} x {eng.H})")
            self._frame = (w_f, h_f, fx, fy, eng.W, eng.H, bool(frame_bgr))
        self._lanes_all = None

    # ------------------------------------------------------------------------------------ frames
    frame_steps = property(lambda self: self.state.frame_steps, doc="steps that ran the frame body (the full window)")
    held_steps = property(lambda self: self.state.held_steps, doc="steps that ran the held body (no image branch)")
    track_ids = property(lambda self: self.state.track_ids, doc="the last step's track ids int64 [B, A] on the device (row "
                         "i of lane b belongs to det[b, i]; 0: no track), valid until the next step; None without track=")
    track_hits = property(lambda self: self.state.track_hits, doc="the last step's hit counts int32 [B, A], as track_ids")
    track_boxes = property(lambda self: self.state.track_boxes, doc="the last step's filtered boxes fp32 [B, A, 4] of a "
                           "motion stream (the track's box behind the update; the row's own box without a track), as "
                           "track_ids; None without motion=")
    track_vel = property(lambda self: self.state.track_vel, doc="the last step's velocities fp32 [B, A, 4] in pixels per "
                         "microsecond per corner (0 without a track), as track_boxes")

    def held_maps(self):
        """The live ``(feats, cnn_out)`` tensors of the frame in force -- what the next held step samples -- or None when
        the next step runs the frame body whatever it brings."""
        return self.model.engine().held_maps(self.state)

    def _push_frame(self, frame, frame_lanes):
        """``frame=`` of a step: raw uint8 frames into the named lanes of the stream's frame buffer, on the device."""
        import torch
        if not self.model.engine().use_image:
            raise ValueError("EventStream: frame= is given to an events-only model (no --use_image): it reads no frame")
        if self._frame is None:
            raise ValueError("EventStream: frame= needs a stream built with frame_size=(W_f, H_f)")
        w_f, h_f, fx, fy, width, height, bgr = self._frame
        if not torch.is_tensor(frame):
            frame = torch.from_numpy(np.ascontiguousarray(np.asarray(frame)))
        if frame.dim() == 3:
            frame = frame[None]
        if frame.dtype != torch.uint8 or frame.dim() != 4 or tuple(frame.shape[1:]) != (h_f, w_f, 3):
            raise ValueError(f"EventStream: frame= is uint8 [n, {h_f}, {w_f}, 3] or [{h_f}, {w_f}, 3] (frame_size), got "
                             f"{frame.dtype} {tuple(frame.shape)}")
        frame = frame.to(self.device)
        if frame.stride(3) != 1 or frame.stride(2) != 3 or frame.stride(1) < 3 * w_f or \
                (frame.shape[0] > 1 and frame.stride(0) < frame.stride(1) * h_f):
            frame = frame.contiguous()                  # (padded rows are taken as they are)
        n = int(frame.shape[0])
        if frame_lanes is None:
            if n != self.B:
                raise ValueError(f"EventStream: frame= holds {n} frames for {self.B} lanes; name their lanes (frame_lanes=)")
            if self._lanes_all is None:
                self._lanes_all = torch.arange(self.B, dtype=torch.int32, device=self.device)
            lanes = self._lanes_all
        else:
            lanes = torch.as_tensor(frame_lanes).to(device=self.device, dtype=torch.int32).reshape(-1).contiguous()
            if lanes.numel() != n:
                raise ValueError(f"EventStream: frame_lanes names {lanes.numel()} lanes for {n} frames")
        self.state.write_frames(frame, lanes, fx, fy, width, height, bgr)

    # ------------------------------------------------------------------------------------ inputs
    def _upload(self, xy, t, p, batch, t_now):
        """The new events on the device as (xy int16[n,2], t int64[n], p int8[n], batch int32/int64[n], t_now int64[B] or
        None).  Host inputs are packed into one buffer: ONE upload, of the new events only."""
        import torch
        tensors = [v for v in (xy, t, p, batch, t_now) if v is not None]
        if all(torch.is_tensor(v) and v.is_cuda for v in tensors):
            n = int(t.shape[0])
            if batch is None:
                if self._zeros is None or self._zeros.shape[0] < n:
                    self._zeros = torch.zeros((max(n, 4096),), dtype=torch.int32, device=self.device)
                batch = self._zeros[:n]
            elif batch.dtype not in (torch.int32, torch.int64):
                batch = batch.to(torch.int32)
            return (xy.to(torch.int16).reshape(-1, 2).contiguous(), t.to(torch.int64).contiguous(),
                    p.to(torch.int8).reshape(-1).contiguous(), batch.contiguous(),
                    None if t_now is None else t_now.to(torch.int64).reshape(-1).contiguous())

        def host(v, dtype):
            return np.ascontiguousarray((v.cpu().numpy() if torch.is_tensor(v) else np.asarray(v)).astype(dtype, copy=False))
        t = host(t, np.int64)
        n = len(t)
        xy = host(xy, np.int16).reshape(-1, 2)
        p = host(p, np.int8).reshape(-1)
        batch = np.zeros(n, np.int32) if batch is None else host(batch, np.int32)
        if not (len(xy) == len(p) == len(batch) == n):
            raise ValueError("EventStream: xy, t, p and batch differ in length")
        now = None if t_now is None else np.broadcast_to(host(t_now, np.int64).reshape(-1), (self.B,))
        o_xy, o_b, o_p = 8 * n, 12 * n, 16 * n
        o_now = (17 * n + 7) // 8 * 8
        buf = np.empty(o_now + 8 * self.B, np.uint8)
        buf[:o_xy] = t.view(np.uint8)
        buf[o_xy:o_b] = xy.reshape(-1).view(np.uint8)
        buf[o_b:o_p] = batch.view(np.uint8)
        buf[o_p:o_p + n] = p.view(np.uint8)
        if now is not None:
            buf[o_now:] = np.ascontiguousarray(now).view(np.uint8)
        d = torch.from_numpy(buf).to(self.device)
        return (d[o_xy:o_b].view(torch.int16).view(-1, 2), d[:o_xy].view(torch.int64), d[o_p:o_p + n].view(torch.int8),
                d[o_b:o_p].view(torch.int32), None if now is None else d[o_now:].view(torch.int64))

    def _frame_and_now(self, t_now, image, frame, frame_lanes):
        """What every kind of step does first: the frames into their lanes, a scalar ``t_now`` for every lane."""
        import torch
        if frame is not None:
            if image is not None:
                raise ValueError("EventStream: image= and frame= are both given; a step takes the model's image batch OR raw "
                                 "frames")
            self._push_frame(frame, frame_lanes)
        elif frame_lanes is not None:
            raise ValueError("EventStream: frame_lanes= is given without frame=")
        if t_now is not None and not torch.is_tensor(t_now) and np.ndim(t_now) == 0:
            t_now = np.full((self.B,), int(t_now), np.int64)
        elif torch.is_tensor(t_now) and t_now.numel() == 1 and self.B > 1:
            t_now = t_now.reshape(1).expand(self.B)
        return t_now

    def _upload_words(self, words, lane_words, t_now):
        """The words of a push on the device as (bit patterns int16 / int32 [n], word_end int64[B], t_now int64[B] or
        None).  Host inputs are packed into one buffer: ONE upload, of word_end, t_now and the words."""
        import torch
        _, dtype, _ = DECODE_FORMATS[self.decode]
        size = np.dtype(dtype).itemsize
        bits = torch.int16 if size == 2 else torch.int32
        if torch.is_tensor(words) and words.is_cuda:
            words = words.reshape(-1).contiguous()
            if words.dtype == torch.uint8:
                if words.numel() % size:
                    raise ValueError(f"EventStream: {words.numel()} bytes are not a whole number of {size}-byte "
                                     f"{self.decode} words")
            elif words.element_size() != size or words.dtype.is_floating_point:
                raise ValueError(f"EventStream: {self.decode} words are {np.dtype(dtype).name} (or bytes / uint8), got "
                                 f"{words.dtype}")
            words = words.view(bits)
            n = int(words.numel())
            if torch.is_tensor(lane_words) and lane_words.is_cuda:
                if lane_words.numel() != self.B:
                    raise ValueError(f"EventStream: lane_words needs one count per lane ({self.B})")
                end = torch.cumsum(lane_words.reshape(-1).to(torch.int64), 0)
            else:
                end = torch.from_numpy(np.cumsum(_lane_words(lane_words, n, self.B, "EventStream"))).to(self.device)
            if t_now is not None and not torch.is_tensor(t_now):
                t_now = torch.from_numpy(np.ascontiguousarray(np.asarray(t_now, np.int64))).to(self.device)
            return words, end, None if t_now is None else t_now.to(device=self.device, dtype=torch.int64).reshape(-1).contiguous()
        if torch.is_tensor(words):
            words = words.cpu().reshape(-1)
            words = words.view(torch.uint8).numpy() if words.dtype == torch.uint8 else words.view(bits).numpy().view(dtype)
        words = words_as_array(words, self.decode, "EventStream")
        n = len(words)
        if torch.is_tensor(lane_words):
            lane_words = lane_words.cpu().numpy()
        end = np.cumsum(_lane_words(lane_words, n, self.B, "EventStream"))
        now = None
        if t_now is not None:
            now = t_now.cpu().numpy() if torch.is_tensor(t_now) else np.asarray(t_now)
            now = np.ascontiguousarray(np.broadcast_to(now.astype(np.int64).reshape(-1), (self.B,)))
        o_now, o_words = 8 * self.B, 16 * self.B
        buf = np.empty(o_words + size * n, np.uint8)
        buf[:o_now] = end.astype(np.int64).view(np.uint8)
        buf[o_now:o_words] = 0 if now is None else now.view(np.uint8)
        buf[o_words:] = words.view(np.uint8)
        d = torch.from_numpy(buf).to(self.device)
        return d[o_words:].view(bits), d[:o_now].view(torch.int64), None if now is None else d[o_now:o_words].view(torch.int64)

    # ------------------------------------------------------------------------------------ steps
    def step_words_device(self, words, lane_words=None, t_now=None, image=None, frame=None, frame_lanes=None):
        """One step of a decoding stream (``decode=``) without a host synchronisation: as ``step_device``, with the camera's
        words in place of the events.  ``words``: uint16 (EVT 3.0) / uint32 (EVT 2.0) words, host or device -- a device
        tensor may hold them as int16 / int32 bit patterns --, or ``bytes`` / a uint8 buffer whose length is a multiple of
        the word size (little-endian).  ``lane_words``: ints ``[B]``, the words of every lane in lane order (default: all
        words to lane 0 when ``B == 1``).  Host inputs travel in ONE upload: the words, their lane ends and ``t_now``."""
        import torch
        if self.decode is None:
            raise ValueError("EventStream: step_words / step_words_device need a stream built with decode='evt2' or 'evt3'; "
                             "this stream takes decoded events (step / step_device)")
        t_now = self._frame_and_now(t_now, image, frame, frame_lanes)
        words, word_end, t_now = self._upload_words(words, lane_words, t_now)
        if t_now is not None and t_now.numel() != self.B:
            raise ValueError(f"EventStream: t_now needs one instant per lane ({self.B})")
        eng = self.model.engine()
        with torch.no_grad():
            self.outputs, det = eng.forward_stream(self.state, None, None, None, None, t_now=t_now, image=image, words=words,
                                                   word_end=word_end)
        self.model._window = None            # a reset=False call then starts from a window of its own
        return det

    def step_words(self, words, lane_words=None, t_now=None, image=None, frame=None, frame_lanes=None):
        """One step of a decoding stream: the detections list ``model(x, reset=True)[0]`` returns for the stream's window."""
        return self._finish_step(self.step_words_device(words, lane_words=lane_words, t_now=t_now, image=image, frame=frame,
                                                        frame_lanes=frame_lanes))

    def decode_counts(self):
        """The decoder's counters since construction / ``reset()``: a dict of ``decoded``, ``unsynced``, ``outside`` and
        ``skipped``, int64 [B] each (synchronises).  Raises without ``decode=``."""
        c = self.state.decode_counts()
        return {k: c[:, i].copy() for i, k in enumerate(DECODE_COUNTERS)}

    def decode_state(self):
        """The lanes' decoder states: a dict of ``high``, ``low``, ``loops``, ``y``, ``base_x``, ``pol`` and ``synced``,
        int64 [B] each (synchronises).  Raises without ``decode=``."""
        s = self.state.decode_state()
        return {k: s[:, i].copy() for i, k in enumerate(DECODE_STATE)}

    def step_device(self, xy, t, p, batch=None, t_now=None, image=None, frame=None, frame_lanes=None):
        """One step without a host synchronisation: ``(det[B, A, 6], n_keep[B])`` as ``forward_detections`` returns them,
        valid until the engine's next call.  ``image``: the model's image batch fp32 [B, 3, H, W]; ``frame``: raw sensor
        frames uint8 ``[n, H_f, W_f, 3]`` or ``[H_f, W_f, 3]`` (host or device) for the lanes ``frame_lanes`` (default: all
        lanes in order) -- the other lanes keep their frame; either makes the step a frame step for the whole batch."""
        import torch
        if self.decode is not None:
            raise ValueError(f"EventStream: step / step_device take decoded events; this stream decodes {self.decode} words "
                             "(decode=): use step_words / step_words_device")
        t_now = self._frame_and_now(t_now, image, frame, frame_lanes)
        xy, t, p, batch, t_now = self._upload(xy, t, p, batch, t_now)
        if t_now is not None and t_now.numel() != self.B:
            raise ValueError(f"EventStream: t_now needs one instant per lane ({self.B})")
        eng = self.model.engine()
        with torch.no_grad():
            self.outputs, det = eng.forward_stream(self.state, xy, t, p, batch, t_now=t_now, image=image)
        self.model._window = None            # a reset=False call then starts from a window of its own
        return det

    def step(self, xy, t, p, batch=None, t_now=None, image=None, frame=None, frame_lanes=None):
        """One step: the detections list ``model(x, reset=True)[0]`` returns for the stream's window."""
        return self._finish_step(self.step_device(xy, t, p, batch=batch, t_now=t_now, image=image, frame=frame,
                                                  frame_lanes=frame_lanes))

    def _finish_step(self, det_n_keep):
        """The read-back that ends ``step`` / ``step_words``."""
        from .model.utils import detections_from_device
        det, n_keep = det_n_keep
        detections = detections_from_device(det, n_keep)        # the step's one synchronisation
        if self.track is not None:                              # cut by the counts that read-back brought
            for name in ("track_ids", "track_hits") + (("track_boxes", "track_vel") if self.motion is not None else ()):
                rows = getattr(self.state, name).clone()
                for b, d in enumerate(detections):
                    d[name] = rows[b, :int(d["scores"].shape[0])]
        self.model.engine().stream_counted(self.state)          # the counts came back with it
        if self.model.check_device_status:
            self.check_status()
        return detections

    def counts(self):
        """Events per lane of the current window (synchronises)."""
        import torch
        torch.cuda.current_stream(self.device).synchronize()
        self.model.engine().stream_counted(self.state)
        known = self.state.counts_known()
        return known if known is not None else np.zeros((self.B,), np.int64)

    def dropped(self):
        """Events per lane the count rule has removed beyond the time rule since construction / ``reset()``: int64 [B],
        zeros for a stream without ``max_lane_events`` (synchronises)."""
        return self.state.dropped()

    def change_maps(self):
        """The lanes' change maps fp32[B, H_in // fy, W_in // fx] of a downsampling stream (a copy; synchronises)."""
        return self.state.change_maps()

    def filtered(self):
        """Events per lane the noise filter has removed since construction / ``reset()``: int64 [B], zeros for a stream
        without ``denoise_us`` / ``refractory_us`` (synchronises)."""
        return self.state.filtered()

    def last_stamps(self):
        """The lanes' stamp maps int64[B, H_in, W_in] of a filtering stream, "never" as ``np.iinfo(np.int64).min`` (a copy;
        synchronises)."""
        return self.state.last_stamps()

    def suppressed(self):
        """Events per lane the flicker stage and the trail stage have removed since construction / ``reset()``:
        ``(flicker int64 [B], trail int64 [B])``, zeros for a stream without ``flicker`` / ``trail_us`` (synchronises)."""
        return self.state.suppressed()

    def flicker_state(self):
        """The per-pixel state of the flicker / trail filters as ``flicker_definition`` names it: a dict of ``t_edge``,
        ``last_p``, ``count``, ``blocking``, ``t_pass`` and ``p_pass`` over ``[B, H_in, W_in]``, "never" as
        ``np.iinfo(np.int64).min`` (copies; synchronises).  Raises without ``flicker`` / ``trail_us``."""
        return self.state.flicker_maps()

    def tracks(self):
        """Per lane the live tracks of a tracking stream, a ``TRACK_DTYPE`` array (``id, x1, y1, x2, y2, label, t_last,
        hits``) sorted by id (copies; synchronises).  A motion stream's arrays are ``TRACK_MOTION_DTYPE``: ``vx1, vy1, vx2,
        vy2`` (pixels per microsecond) appended."""
        *slots, _ = self.state.track_slots()                    # id, t_last, box, (vel,) label, hits; next_id
        vel = slots.pop(3) if self.motion is not None else [None] * self.B
        return [tracks_from_arrays(*(a[b] for a in slots), vel[b]) for b in range(self.B)]

    def coast_device(self):
        """The last step's coast lists of a motion stream as the raw device tensors ``(n_coast int32 [B], coast_id int64
        [B, max_tracks], coast_box fp32 [B, max_tracks, 4], coast_label int32 [B, max_tracks], coast_age_us int64
        [B, max_tracks])``: the first ``n_coast[b]`` entries of lane ``b`` are the step's, valid until the next step."""
        return self.state.coast_device()

    def coasting(self):
        """Per lane the tracks the last step did not see, where they are predicted to be at the step's ``t_ref``: a
        ``COAST_DTYPE`` array (``id, x1, y1, x2, y2, label, age_us``) in slot order (copies; synchronises)."""
        n, ids, box, label, age = (t.cpu().numpy() for t in self.state.coast_device())
        return [coast_from_arrays(int(n[b]), ids[b], box[b], label[b], age[b]) for b in range(self.B)]

    def untracked(self):
        """Eligible rows per lane that got no track id since construction / ``reset()`` -- beyond the first
        ``DAGR_TRACK_MAX_DETS`` of a step, or unmatched with every slot taken: int64 [B] (synchronises)."""
        return self.state.untracked()

    def rescued(self):
        """Matches of the second association round per lane since construction / ``reset()``: rows under ``min_score``
        that continued a track: int64 [B] (synchronises).  Raises without ``rescue=``."""
        return self.state.rescued()

    def render_step(self, base=None, out=None):
        """The lanes' frames of the last step, uint8 BGR ``[B, H, W, 3]`` on the device (class docstring; needs
        ``render=``): ``dagr_stream_render`` on the stream's own arrays, no host wait.  ``base``: a uint8 BGR device tensor
        ``[B, H, W, 3]`` or ``[H, W, 3]`` (one image under every lane) to paint on; without it the base is black.  ``out``
        (default: the stream's own frames) may be ``base`` itself.  The result is valid until the next ``render_step``.  It
        may be called after any step, any number of times -- two calls after one step give equal frames --, and before the
        first step it returns the base.  What it draws are the arrays the last step left, so it belongs in front of the
        engine's next call."""
        import torch
        if self.render is None:
            raise RuntimeError("EventStream: this stream draws nothing (render=): it has no render_step")
        eng = self.model.engine()
        shape, stride = (self.B, eng.H, eng.W, 3), 0
        for name, v in (("base", base), ("out", out)):
            if v is None:
                continue
            ok = torch.is_tensor(v) and v.dtype == torch.uint8 and v.device == self.device and v.is_contiguous() and \
                (tuple(v.shape) == shape or (name == "base" and tuple(v.shape) == shape[1:]))
            if not ok:
                raise ValueError(f"EventStream: render_step {name}= is a contiguous uint8 {list(shape)}"
                                 + (f" or {list(shape[1:])}" if name == "base" else "") + f" tensor on {self.device}")
        if base is not None:
            stride = eng.H * eng.W * 3 if base.dim() == 4 else 0
            if stride == 0 and self.B > 1 and out is not None and out.data_ptr() == base.data_ptr():
                raise ValueError("EventStream: render_step out= cannot be a base= that every lane shares")
        return self.state.run_render(base, stride, out)

    def trails(self):
        """The trail rings of a drawing stream with ``trail > 0``, per lane a dict of track id -> int32 ``[n, 2]`` centres
        ``(x, y)``, oldest first (copies; synchronises)."""
        ids, counts, pts = self.state.trail_arrays()
        T, out = self.render["trail"], []
        for b in range(self.B):
            lane = {}
            for s in np.nonzero(ids[b])[0]:
                c = int(counts[b, s])
                lane[int(ids[b, s])] = pts[b, s, :c].copy() if c <= T else pts[b, s, (c + np.arange(T)) % T]
            out.append(lane)
        return out

    def render_status(self):
        """The picture's flags since the last call, as a list of their descriptions (``RENDER_STATUS_BITS``); the word is
        cleared (synchronises)."""
        if self.render is None:
            raise RuntimeError("EventStream: this stream draws nothing (render=): it has no render_status")
        flag = int(self.state.render_flags.item())
        self.state.render_flags.zero_()
        return [text for bit, text in RENDER_STATUS_BITS if flag & bit]

    def push_labels(self, t, xywh, label, id, n=None, lanes=None):
        """Labelled keyframes into the lanes' stores (module docstring; needs ``labels=``): ONE launch
        (``dagr_stream_labels_push``), no host wait.  ``t`` int64 ``[L]`` and ``xywh`` fp64 ``[L, rows, 4]`` (top-left plus
        size), ``label`` int32 ``[L, rows]``, ``id`` int64 ``[L, rows]`` (``labels_from_tracks`` makes them of a DSEC track
        array) are one keyframe per lane; with a further axis ``F`` behind ``L`` -- ``t [L, F]``, ``xywh [L, F, rows, 4]`` --
        every lane takes ``F`` keyframes in order.  ``n`` int32 ``[L]`` / ``[L, F]``: the rows that count (``None``: all;
        negative: no keyframe for that lane).  ``L`` is the batch size, or the length of ``lanes`` (distinct lane indices);
        the other lanes get nothing.  numpy arrays (uploaded) or device tensors.  The rules -- a keyframe not later than
        the lane's newest is refused, rows beyond ``max_rows`` are cut, a full ring loses its oldest keyframe -- are
        applied and counted on the device (``label_counts()``); host arrays are also checked here: an instant that is not
        greater than the one before it in the call, or than the newest a host push has offered that lane, raises by
        name."""
        import torch
        if self.labels is None:
            raise RuntimeError("EventStream: push_labels needs a stream built with labels=")
        R = self.labels["max_rows"]
        host = not any(torch.is_tensor(v) for v in (t, xywh, label, id, n))

        def ten(v, dtype):
            if not torch.is_tensor(v):
                v = torch.from_numpy(np.ascontiguousarray(np.asarray(v)))
            return v.to(dtype=dtype)
        t, xywh, label, id = ten(t, torch.int64), ten(xywh, torch.float64), ten(label, torch.int32), ten(id, torch.int64)
        n = None if n is None else ten(n, torch.int32)
        if t.dim() == 1:
            t, xywh, label, id = t[:, None], xywh[:, None], label[:, None], id[:, None]
            n = n if n is None or n.dim() != 1 else n[:, None]
        which = list(range(self.B)) if lanes is None else [int(b) for b in np.asarray(lanes).reshape(-1)]
        if sorted(set(which)) != sorted(which) or any(not 0 <= b < self.B for b in which):
            raise ValueError(f"EventStream: push_labels lanes = {which} must be distinct lanes in 0..{self.B - 1}")
        L, F = len(which), int(t.shape[1]) if t.dim() == 2 else -1
        rows = int(xywh.shape[2]) if xywh.dim() == 4 else -1
        if n is None:
            n = torch.full((L, max(F, 0)), max(rows, 0), dtype=torch.int32)
        if tuple(t.shape) != (L, F) or F < 1 or tuple(xywh.shape) != (L, F, rows, 4) or tuple(label.shape) != (L, F, rows) or \
                tuple(id.shape) != (L, F, rows) or tuple(n.shape) != (L, F):
            raise ValueError(f"EventStream: push_labels takes t int64 [{L}] or [{L}, F], xywh fp64 [{L}, (F,) rows, 4], label "
                             f"int32 and id int64 [{L}, (F,) rows] and n int32 like t, got {tuple(t.shape)}, "
                             f"{tuple(xywh.shape)}, {tuple(label.shape)}, {tuple(id.shape)} and {tuple(n.shape)}")
        if host:
            th, nh, newest = t.numpy(), n.numpy(), list(self._label_newest)
            if (nh > rows).any():
                raise ValueError(f"EventStream: push_labels n = {int(nh.max())} exceeds the {rows} rows given")
            for i, b in enumerate(which):
                for f in range(F):
                    if nh[i, f] < 0:
                        continue
                    if newest[b] is not None and int(th[i, f]) <= newest[b]:
                        raise ValueError(f"EventStream: push_labels t = {int(th[i, f])} of lane {b} is not greater than the "
                                         f"lane's newest keyframe instant {newest[b]}: keyframes are pushed in increasing time")
                    newest[b] = int(th[i, f])
            self._label_newest = newest
        dev = self.device
        t, n, xywh, label, id = (v.to(dev) for v in (t, n, xywh, label, id))
        if rows > R:
            xywh, label, id = xywh[:, :, :R], label[:, :, :R], id[:, :, :R]
        elif rows < R:
            pad = lambda v: torch.cat([v, v.new_zeros((L, F, R - rows) + tuple(v.shape[3:]))], dim=2)      # noqa: E731
            xywh, label, id = pad(xywh), pad(label), pad(id)
        if lanes is not None:
            at = torch.as_tensor(which, dtype=torch.int64, device=dev)
            full = [torch.zeros((self.B,) + tuple(v.shape[1:]), dtype=v.dtype, device=dev) for v in (t, n, xywh, label, id)]
            full[1].fill_(-1)
            for whole, part in zip(full, (t, n, xywh, label, id)):
                whole[at] = part
            t, n, xywh, label, id = full
        self.state.push_labels(*(v.contiguous() for v in (t, n, xywh, label, id)))

    def labels_step(self):
        """The ground truth of the LAST step, interpolated to the step's own ``t_ref`` on the device (module docstring;
        needs ``labels=``): ``(gt_box fp32 [B, G, 4] as x1 y1 x2 y2, gt_label int32 [B, G], gt_id int64 [B, G], n_gt int32
        [B])`` with ``G = max_rows``, device tensors valid until the next step -- what ``score_step`` takes, and what a
        caller that evaluates mAP can hand on.  ``n_gt[b] = -1``: lane ``b`` has no labels at this instant; rows at and
        behind ``n_gt[b]`` mean nothing.  ONE launch (``dagr_stream_labels_at``) at most once per step -- asked again, it
        returns the same tensors --, no host wait.  Raises by name before the stream's first step."""
        if self.labels is None:
            raise RuntimeError("EventStream: labels_step needs a stream built with labels=")
        return self.state.run_labels()

    def label_counts(self):
        """The label store's counters since construction / ``reset()``: a dict of int64 ``[B]`` per name of
        ``LABEL_COUNTERS`` (``refused``, ``cut_rows``, ``overwritten``, ``labelled``, ``outside``, ``gap``) plus
        ``keyframes``, the resident keyframes.  Synchronises.  Raises without ``labels=``."""
        if self.labels is None:
            raise RuntimeError("EventStream: label_counts needs a stream built with labels=")
        words = self.state.label_words()
        return {name: words[:, i].copy() for i, name in enumerate(LABEL_WORDS) if name != "head"}

    def score_step(self, gt_box=None, gt_label=None, gt_id=None, n_gt=None):
        """Score the LAST step's track ids against labelled boxes, on the device (module docstring; needs ``score=``).
        Without arguments, on a stream with ``labels=``: against the ground truth interpolated to the step's own ``t_ref``
        -- ``labels_step()`` if the step has not had one (``dagr_stream_labels_at``, once), then the unchanged chain on
        its tensors; raises by name on a stream without ``labels=`` or without ``score=``.  With arguments, as ever:
        ``gt_box`` fp32 ``[B, G, 4]`` (x1, y1, x2, y2), ``gt_label`` int32 ``[B, G]``, ``gt_id`` int64 ``[B, G]`` (the
        identities, > 0) and ``n_gt`` int32 ``[B]`` -- ``None``: every lane has all ``G`` rows; ``n_gt[b] < 0``: lane ``b``
        has no labels at this instant and is skipped --, numpy arrays (uploaded) or device tensors,
        ``G <= DAGR_SCORE_MAX_GT``.  ONE launch (``dagr_stream_score``; with ``identity=`` a second,
        ``dagr_stream_identity``, behind it; with ``hota=`` a third, ``dagr_stream_hota``) on the step's own device arrays,
        no host wait.
        Returns ``(gt_match int64 [B, G], gt_flags int32 [B, G])``, device tensors valid until the next ``score_step``:
        per row the track id (0: a miss, -1: unscored) and the bits switch (1), fragmentation (2), kept (4).  Raises by name
        before the stream's first step, when called twice for one step, and on a stream without ``score=``."""
        import torch
        if self.score is None:
            raise RuntimeError("EventStream: score_step needs a stream built with score= (and track=)")
        if gt_box is None:
            if gt_label is not None or gt_id is not None or n_gt is not None:
                raise ValueError("EventStream: score_step takes gt_box, gt_label and gt_id together, or nothing at all (a "
                                 "stream with labels=)")
            if self.labels is None:
                raise RuntimeError("EventStream: score_step() without arguments needs a stream built with labels= (it scores "
                                   "against the interpolated keyframes)")
            return self.state.run_score(*self.state.run_labels())

        def dev(v, dtype, shape, name):
            if not torch.is_tensor(v):
                v = torch.from_numpy(np.ascontiguousarray(np.asarray(v)))
            v = v.to(device=self.device, dtype=dtype).contiguous()
            if shape is not None and tuple(v.shape) != shape:
                raise ValueError(f"EventStream: score_step {name} has shape {tuple(v.shape)}, expected {shape}")
            return v
        G = int(gt_box.shape[1]) if np.ndim(gt_box) == 3 else -1
        if not 0 <= G <= DAGR_SCORE_MAX_GT:
            raise ValueError(f"EventStream: score_step gt_box is fp32 [{self.B}, G, 4] with G <= DAGR_SCORE_MAX_GT = "
                             f"{DAGR_SCORE_MAX_GT}, got {tuple(np.shape(gt_box))}")
        gt_box = dev(gt_box, torch.float32, (self.B, G, 4), "gt_box")
        gt_label = dev(gt_label, torch.int32, (self.B, G), "gt_label")
        gt_id = dev(gt_id, torch.int64, (self.B, G), "gt_id")
        n_gt = torch.full((self.B,), G, dtype=torch.int32, device=self.device) if n_gt is None else \
            dev(n_gt, torch.int32, (self.B,), "n_gt")
        return self.state.run_score(gt_box, gt_label, gt_id, n_gt)

    def track_score(self):
        """The scorer's counters since construction / ``reset()``: a dict of int64 ``[B]`` per name of ``SCORE_COUNTERS``
        (``steps``, ``gt``, ``hyp``, ``match``, ``miss``, ``false_pos``, ``switch``, ``frag``, ``kept``, ``iou_q``,
        ``unscored_gt``, ``unscored_hyp``).  Synchronises.  Raises without ``score=``."""
        _, words = self.state.score_words()
        return {name: words[:, 1 + i].copy() for i, name in enumerate(SCORE_COUNTERS)}

    def scored_objects(self):
        """The scorer's object tables: per lane a ``SCORE_OBJECT_DTYPE`` array (``id, last_hyp, prev_hyp, seen_step,
        present, tracked, switches, frags``) in order of first appearance (copies; synchronises).  ``score_summary`` takes
        ``track_score()`` and this.  Raises without ``score=``."""
        table, words = self.state.score_words()
        return [objects_from_arrays(int(words[b, 0]), *table[:, b]) for b in range(self.B)]

    def identity(self):
        """IDF1's integers for everything scored since construction / ``reset()`` (module docstring; needs ``identity=``): one
        launch (``dagr_stream_identity_solve``: the maximum-weight pairing of object identities with track ids on the
        lanes' overlap counts), then the read-back (synchronises).  Returns a dict of int64 ``[B]`` per name of
        ``IDENTITY_RESULT`` (``idtp``, ``idfn``, ``idfp``, ``gt_frames``, ``hyp_frames``, ``n_objects``, ``n_tracks``,
        ``dup_hyp``, ``unlisted_hyp``) plus ``obj_track``, per lane int64 ``[n_objects]``: the track id paired with the
        object of a slot of ``scored_objects()``, 0 for none.  The counts go on: it can be asked for at any step.
        ``identity_summary`` takes the result."""
        if self.identity_options is None:
            raise RuntimeError("EventStream: identity() needs a stream built with identity= (and score=, track=)")
        result, obj_track = self.state.run_identity_solve()
        result, obj_track = result.cpu().numpy(), obj_track.cpu().numpy()
        out = {name: result[:, i].copy() for i, name in enumerate(IDENTITY_RESULT)}
        out["obj_track"] = [obj_track[b, :int(out["n_objects"][b])].copy() for b in range(self.B)]
        return out

    def identity_tables(self):
        """The identity state read back (copies; synchronises; needs ``identity=``): ``dict(track_id int64 [B, max_tracks],
        track_len int64 [B, max_tracks], obj_len int64 [B, max_objects], overlap int32 [B, max_objects, max_tracks], words:
        a dict of int64 [B] per name of IDENTITY_WORDS)``."""
        if self.identity_options is None:
            raise RuntimeError("EventStream: identity_tables() needs a stream built with identity= (and score=, track=)")
        t = self.state.identity_words()
        return dict(track_id=t["track_id"].copy(), track_len=t["track_len"].copy(), obj_len=t["obj_len"].copy(),
                    overlap=t["overlap"].copy(), words={name: t["words"][:, i].copy() for i, name in enumerate(IDENTITY_WORDS)})

    def hota(self):
        """HOTA's integers and sums for the labelled instants logged since construction / ``reset()`` (module docstring;
        needs ``hota=``): ``dagr_stream_hota_solve`` -- pass 2 over the lanes' logs with the tables as they are now, then the
        fp64 sums --, then the read-back (synchronises).  Returns a dict of ``tp``, ``fn``, ``fp``, ``loc_q`` (int64
        ``[B, 19]``, threshold ``k`` at index ``k - 1``), ``ass``, ``re``, ``pr`` (fp64 ``[B, 19]``) and one int64 ``[B]`` per
        name of ``HOTA_WORDS`` (``instants``, ``dropped_instants``, ``rows``, ``columns``).  The log and the tables go on: it
        can be asked for at any step and repeated.  ``hota_summary`` takes the result."""
        if self.hota_options is None:
            raise RuntimeError("EventStream: hota() needs a stream built with hota= (and identity=, score=, track=)")
        self.state.run_hota_solve()
        t = self.state.hota_words(("words", "count", "sums"))
        out = {name: t["count"][:, :, i].copy() for i, name in enumerate(HOTA_COUNTERS)}
        out.update({name: t["sums"][:, :, i].copy() for i, name in enumerate(HOTA_SUMS)})
        out.update({name: t["words"][:, i].copy() for i, name in enumerate(HOTA_WORDS)})
        return out

    def hota_tables(self):
        """HOTA's state read back (copies; synchronises; needs ``hota=``): ``dict(pmc int64 [B, max_objects, max_tracks], gc
        int64 [B, max_objects], tc int64 [B, max_tracks], mc int32 [B, 19, max_objects, max_tracks] -- the last ``hota()``'s --,
        words: a dict of int64 [B] per name of HOTA_WORDS)``."""
        if self.hota_options is None:
            raise RuntimeError("EventStream: hota_tables() needs a stream built with hota= (and identity=, score=, track=)")
        t = self.state.hota_words(("pmc", "gc", "tc", "mc", "words"))
        return dict(pmc=t["pmc"], gc=t["gc"], tc=t["tc"], mc=t["mc"],
                    words={name: t["words"][:, i].copy() for i, name in enumerate(HOTA_WORDS)})

    def map_step(self, gt_box=None, gt_label=None, n_gt=None):
        """Log the LAST step's detections and ground truth for the COCO protocol, on the device (module docstring; needs
        ``map=``).  Without arguments, on a stream with ``labels=``: against the ground truth interpolated to the step's own
        ``t_ref`` -- ``labels_step()`` if the step has not had one (a ``score_step()`` without arguments has), then the log
        launch; raises by name on a stream without ``labels=``.  With arguments: ``gt_box`` fp32 ``[B, G, 4]`` (x1, y1, x2,
        y2), ``gt_label`` int32 ``[B, G]`` and ``n_gt`` int32 ``[B]`` -- ``None``: every lane has all ``G`` rows; ``n_gt[b] <
        0``: lane ``b`` has no labels at this instant --, numpy arrays (uploaded) or device tensors, ``G <=
        DAGR_COCO_MAX_GT``, the same ``G`` at every call.  ONE launch (``dagr_stream_map_log``), no host wait; returns
        nothing.  Raises by name before the stream's first step and when called twice for one step."""
        import torch
        if self.map_options is None:
            raise RuntimeError("EventStream: map_step needs a stream built with map=")
        if gt_box is None:
            if gt_label is not None or n_gt is not None:
                raise ValueError("EventStream: map_step takes gt_box and gt_label together, or nothing at all (a stream with "
                                 "labels=)")
            if self.labels is None:
                raise RuntimeError("EventStream: map_step() without arguments needs a stream built with labels= (it logs the "
                                   "interpolated keyframes)")
            box, label, _, n = self.state.run_labels()
            return self.state.run_map_log(box, label, n)

        def dev(v, dtype, shape, name):
            if not torch.is_tensor(v):
                v = torch.from_numpy(np.ascontiguousarray(np.asarray(v)))
            v = v.to(device=self.device, dtype=dtype).contiguous()
            if tuple(v.shape) != shape:
                raise ValueError(f"EventStream: map_step {name} has shape {tuple(v.shape)}, expected {shape}")
            return v
        G = int(gt_box.shape[1]) if np.ndim(gt_box) == 3 else -1
        if not 1 <= G <= DAGR_COCO_MAX_GT:
            raise ValueError(f"EventStream: map_step gt_box is fp32 [{self.B}, G, 4] with 1 <= G <= DAGR_COCO_MAX_GT = "
                             f"{DAGR_COCO_MAX_GT}, got {tuple(np.shape(gt_box))}")
        gt_box = dev(gt_box, torch.float32, (self.B, G, 4), "gt_box")
        gt_label = dev(gt_label, torch.int32, (self.B, G), "gt_label")
        n_gt = torch.full((self.B,), G, dtype=torch.int32, device=self.device) if n_gt is None else \
            dev(n_gt, torch.int32, (self.B,), "n_gt")
        self.state.run_map_log(gt_box, gt_label, n_gt)

    def map(self):
        """COCO mAP over everything logged since construction / ``reset()`` (module docstring; needs ``map=``):
        ``dagr_stream_map_plan`` builds the protocol's job list from the log on the device, the totals block comes back (one
        small copy: the C entries of match and accumulate take host sizes), then ``dagr_coco_match``, ``group_ngt`` from
        ``g_ign``, ``score_order`` and ``dagr_coco_accumulate`` run on the plan's arrays where they lie, and only the
        precision array, the two status words and the lanes' words are copied back (synchronises).  Returns the dict
        ``evaluate_detection`` returns -- ``AP``, ``AP_50``, ``AP_75``, ``AP_S``, ``AP_M``, ``AP_L``; all zero when no
        detection was logged -- plus one int64 ``[B]`` per name of ``MAP_WORDS`` (``images``, ``dropped_images``,
        ``cut_dets``, ``unlabelled``, ``empty``).  The log goes on: it can be asked for at any step and repeated."""
        from .utils.coco_eval import OUT_KEYS, summarize
        if self.map_options is None:
            raise RuntimeError("EventStream: map() needs a stream built with map=")
        plan = self.state.run_map_plan()
        if plan is None:                                            # nothing was ever logged
            words, out = self.state.map_words(), {k: 0 for k in OUT_KEYS}
        else:
            n_words = 8 * len(MAP_WORDS) * self.B
            _, prec, back = plan.precision(also=self.state.map_state[:n_words])
            words = back.view(np.int64).reshape(self.B, len(MAP_WORDS))
            out = {k: 0 for k in OUT_KEYS} if prec is None else summarize(prec)
        out.update({name: words[:, i].copy() for i, name in enumerate(MAP_WORDS)})
        return out

    def map_counts(self):
        """The log's counters since construction / ``reset()``: a dict of int64 ``[B]`` per name of ``MAP_WORDS``.
        Synchronises.  Raises without ``map=``."""
        if self.map_options is None:
            raise RuntimeError("EventStream: map_counts needs a stream built with map=")
        words = self.state.map_words()
        return {name: words[:, i].copy() for i, name in enumerate(MAP_WORDS)}

    def map_log(self):
        """The log read back (copies; synchronises; needs ``map=``): per lane the list of its images in log order as ``(t,
        gt_box fp32 [g, 4], gt_label int32 [g], det fp32 [d, 6])`` -- ``MapDefinition.log``'s shape."""
        if self.map_options is None:
            raise RuntimeError("EventStream: map_log needs a stream built with map=")
        words, arrays = self.state.map_words(log=True)
        if arrays is None:
            return [[] for _ in range(self.B)]
        return [[(int(arrays["t"][b, k]), arrays["gt_box"][b, k, :arrays["n_gt"][b, k]], arrays["gt_label"][b, k, :arrays["n_gt"][b, k]],
                  arrays["det"][b, k, :arrays["n_dt"][b, k]]) for k in range(int(words[b, 0]))] for b in range(self.B)]

    def reset(self):
        """Empty the stream: no resident events, no reference instants, zero change maps, empty stamp maps, every pixel of
        the flicker / trail filters in its initial state, zero dropped, filtered and suppressed counts, zero decoder states and counters, a clear status word, zero step counters; no tracks, ids from 1 again, zero untracked and rescued counts; the
        scorer's object tables empty and its counters zero (and no step left to score); the identity state and HOTA's state and log empty; the label
        store empty and its counters zero; the mAP log empty and its counters zero; the trail rings empty, the picture's flags clear and no step left to draw.  The
        frame in force stays, and the next step runs it through the image branch again."""
        self.state.reset()
        self._label_newest = [None] * self.B

    def check_status(self):
        """Raise ``RuntimeError`` naming the stream's flag if a step raised one (the word is cleared: the stream goes on
        from whatever the flagged step left), then the engine's own ``check_status``.  Synchronises."""
        flag = int(self.state.status.item())
        if flag:
            self.state.status.zero_()
            raise RuntimeError(f"event stream flagged {flag:#x}: {_flag_names(flag)}")
        self.model.engine().check_status()
