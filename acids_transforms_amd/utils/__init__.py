from .misc import *  # noqa
from .heapq import heappush, heappop  # noqa
from .audio_io import Resample, RealtimeResample, resample, import_data, load_wav  # noqa
from . import filter_design  # noqa  (host-side designs of second-order sections for transforms.SOSFilter)
