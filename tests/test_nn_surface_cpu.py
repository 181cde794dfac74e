"""nn.py after the split into topic modules: every name it exposed before is still there, every moved class and function is defined
once, in its topic module, and the topic modules import neither nn nor engine nor ops."""
import importlib
import inspect
import os
import subprocess
import sys

from mlperf_deepcam_amd import nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the non-module names of nn before the split
SURFACE = (
    'Adam', 'AdamW', 'ArenaOptimizer', 'CLASS_FREQ', 'CLIMATOLOGY_GROUPS', 'CLIMATOLOGY_MAX_FRAMES', 'CLIMATOLOGY_PRODUCTS', 'CLIMATOLOGY_ROWS',
    'COMPOSITE_COUNTS', 'COMPOSITE_KEYS', 'COMPOSITE_MAX_EVENTS', 'COMPOSITE_MAX_RADIUS', 'Climatology', 'DECISION_COUNTS', 'DECISION_NEVER',
    'DISPLACEMENT_MAX_BATCH', 'DISPLACEMENT_MAX_RADIUS', 'DISPLACEMENT_RADIUS', 'DISTANCE_MAX_BATCH', 'DISTANCE_MAX_RADIUS', 'DISTANCE_Q',
    'DISTANCE_RADIUS', 'DecisionRule', 'DeepLabv3_plus', 'Dict', 'DisplacementSkill', 'DistanceSkill', 'EARTH_RADIUS_KM', 'ENSEMBLE_CHANGED',
    'ENSEMBLE_MAX_MEMBERS', 'ENSEMBLE_MAX_WEIGHT_SUM', 'ENSEMBLE_ROW', 'EVENT_FIELDS', 'EVENT_FIELD_STATS', 'EVENT_FILTER_COUNTS', 'EVENT_SCALE',
    'EVENT_SHAPE_FIELDS', 'EVENT_SHAPE_VALUES', 'Engine', 'EventCatalog', 'EventFields', 'EventFilter', 'EventMatcher', 'EventShape',
    'EventTracker', 'FSS_MAX_BATCH', 'FSS_MAX_WINDOW', 'FSS_MAX_WINDOWS', 'FSS_WINDOWS', 'Fraction', 'FractionsSkill', 'FrameRenderer',
    'GradualWarmupScheduler', 'LAMB', 'List', 'MultiStepSchedule', 'Optional', 'OrderedDict', 'PROB_BINS', 'PROB_MAX_BATCH', 'PROB_MAX_BINS',
    'PROB_MAX_PIXELS', 'PROB_ONE', 'Predictor', 'ProbabilitySkill', 'RENDER_BACKGROUND', 'RENDER_COLOURS', 'SCALE_LISTS', 'SCALE_MAX_BATCH',
    'SCALE_MAX_LEVELS', 'SCALE_MAX_ORIGINS', 'ScaleSkill', 'Sequence', 'StormComposite', 'TRACK_FIELDS', 'TRACK_FIELD_STATS',
    'TRACK_STEP_FIELDS', 'TRACK_STORE_FIELDS', 'TrackFields', 'TrainStep', 'ValStep', 'ViewEnsemble', '_BYTES', '_DATE', '_FpLoss',
    '_MaskSkill', '_NetFn', '_RAMP', '_SEASON_OF_MONTH', '_c_int', '_cw_cache', '_cw_tensor', '_dlogits_for', '_filled_rows', '_float', '_fss',
    '_n_valid', '_ratio', '_scale_components', '_two_words', 'annotations', 'brier_from_rows', 'class_weights', 'climatology_group',
    'composite_bits', 'composite_radius_table', 'compute_score', 'decision_q', 'decision_q_from_bin', 'displacement_best',
    'displacement_from_rows', 'distance_from_rows', 'distance_table', 'event_field_bits', 'event_field_key', 'event_field_value',
    'event_shape_tables', 'event_weight_tables', 'fp_loss', 'fss_from_rows', 'gall_rows', 'get_lr_schedule', 'graticule', 'iou_from_counts',
    'make_optimizer', 'plate_rows', 'predict_from_logits', 'render_palette', 'scale_from_rows', 'scale_levels', 'seam_weights', 'view_input',
    'wce_fused')

# the classes and functions among them that moved, by their new home
HOME = {
    "events": ('EventCatalog', 'EventFields', 'EventFilter', 'EventMatcher', 'EventShape', 'EventTracker', 'TrackFields', '_filled_rows',
               'event_field_bits', 'event_field_key', 'event_field_value', 'event_shape_tables', 'event_weight_tables'),
    "render": ('FrameRenderer', 'gall_rows', 'graticule', 'plate_rows', 'render_palette'),
    "climate": ('Climatology', 'StormComposite', 'climatology_group', 'composite_bits', 'composite_radius_table'),
    "skills": ('DisplacementSkill', 'DistanceSkill', 'FractionsSkill', 'ProbabilitySkill', 'ScaleSkill', '_MaskSkill', '_fss',
               '_scale_components', 'brier_from_rows', 'displacement_best', 'displacement_from_rows', 'distance_from_rows', 'distance_table',
               'fss_from_rows', 'scale_from_rows', 'scale_levels'),
    "decide": ('DecisionRule', 'ViewEnsemble', 'decision_q', 'decision_q_from_bin', 'seam_weights', 'view_input'),
    "_args": ('_c_int', '_float', '_n_valid', '_ratio', '_two_words'),
}


def test_every_name_of_the_old_surface_is_still_an_attribute():
    assert len(SURFACE) == 133 and len(set(SURFACE)) == 133
    missing = [n for n in SURFACE if not hasattr(nn, n)]
    assert not missing, missing


def test_moved_classes_and_functions_are_defined_once_in_their_topic_module():
    moved = [name for names in HOME.values() for name in names]
    assert len(moved) == 50 and len(set(moved)) == 50 and set(moved) <= set(SURFACE)
    for module, names in HOME.items():
        home = importlib.import_module("mlperf_deepcam_amd." + module)
        for name in names:
            obj = getattr(nn, name)
            assert inspect.isclass(obj) or inspect.isfunction(obj), name
            assert obj is getattr(home, name), name
            assert obj.__module__ == home.__name__, (name, obj.__module__)
    # HOME leaves out none of the surface's classes and functions that live in a topic module
    topic = {"mlperf_deepcam_amd." + module for module in HOME}
    objs = {name: getattr(nn, name) for name in SURFACE}
    found = {name for name, obj in objs.items() if (inspect.isclass(obj) or inspect.isfunction(obj)) and obj.__module__ in topic}
    assert found == set(moved), found ^ set(moved)


def test_topic_modules_import_neither_nn_nor_engine_nor_ops():
    # one fresh child interpreter per module, started together
    code = ("import importlib, sys\n"
            "importlib.import_module('mlperf_deepcam_amd.' + sys.argv[1])\n"
            "print([m for m in ('nn', 'engine', 'ops') if 'mlperf_deepcam_amd.' + m in sys.modules])\n")
    children = {name: subprocess.Popen([sys.executable, "-c", code, name], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
                for name in HOME}
    for name, child in children.items():
        out, err = child.communicate(timeout=120)
        assert child.returncode == 0, (name, err[-2000:])
        assert out.strip() == "[]", (name, out)
