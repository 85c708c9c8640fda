"""The committed slice of the all-against-all sweep: SLICE_SEEDS x SLICE_CASES cases of tests/_pairs_fuzz.py, CHUNK to
an item, each dispatched to its cmpr_hamming_* / cmpr_edit_* / cmpr_tcrdist_* entry point (host or _device) and
compared with the yardsticks for exact equality (tests/_pairs_fuzz_call.py).  tests/test_pairs_fuzz_cpu.py proves on
the CPU that these cases are not vacuous.  A failure prints the case in full, the first differing element and the line
that replays it alone; the long sweep with other seeds is run by hand (tests/fuzz_pairs_gpu.py)."""

import pytest

import _pairs_fuzz as pf
import _pairs_fuzz_call
from compairr_amd import HipError

pytestmark = pytest.mark.gpu

CMPR_EINVAL, CMPR_EUNSUPPORTED = 1, 4

ITEMS = [(seed, first) for seed in pf.SLICE_SEEDS for first in range(0, pf.SLICE_CASES, pf.CHUNK)]


@pytest.mark.parametrize("seed,first", ITEMS, ids=["%d-%d" % item for item in ITEMS])
def test_slice(seed, first):
    assert len(ITEMS) == 12
    for index in range(first, first + pf.CHUNK):
        try:
            _pairs_fuzz_call.run_case(pf.case(seed, index))
        except HipError as e:
            if e.code not in (CMPR_EINVAL, CMPR_EUNSUPPORTED):         # the device failed: nothing more runs on it
                pytest.exit("test_slice[%d-%d], case %d: %s" % (seed, first, index, e), returncode=1)
            raise
