"""Detection visualisation (reference: src/dagr/visualization/), drawn on the device by csrc/viz.hip.

``event_viz.draw_events_on_image`` and ``bbox_viz.filter_boxes`` / ``draw_bbox_on_img`` keep the reference's signatures;
``frames.render_frames`` draws many frames per device call (scripts/visualize_detections.py).
"""
from .frames import render_frames  # noqa: F401
