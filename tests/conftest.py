import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs a real MI355X (run with -m gpu on the GPU box)")


@pytest.fixture(scope="session")
def oracle():
    import oraclelib

    return oraclelib.Oracle()


_REFERENCE_LOGS = {}


@pytest.fixture(scope="session")
def live_reference():
    import oraclelib

    return oraclelib.Reference() if oraclelib.Reference.available() else None


@pytest.fixture
def reference(request, live_reference):
    """The compiled reference (oracle/_ref/libmcref.so) where it was built; elsewhere its recorded answers to the
    same calls (tests/golden/reference_outputs.npz).  MCRT_RECORD_REFERENCE=1 records them anew from the former."""
    import oraclelib

    if os.environ.get("MCRT_RECORD_REFERENCE") == "1":
        if live_reference is None:
            pytest.fail("MCRT_RECORD_REFERENCE=1 needs the compiled reference (oracle/_ref/libmcref.so)")
        return oraclelib.RecordingReference(live_reference, _REFERENCE_LOGS.setdefault(request.node.name, []))
    if live_reference is not None:
        return live_reference
    return oraclelib.ReplayReference(request.node.name)


def pytest_sessionfinish(session, exitstatus):
    if _REFERENCE_LOGS and exitstatus == 0:
        import oraclelib

        oraclelib.write_reference_outputs(_REFERENCE_LOGS)


@pytest.fixture(scope="session")
def mcrt():
    import minecraftskin_raytracer_amd as M

    return M


@pytest.fixture(scope="session")
def gpu(mcrt):
    if mcrt.device_count() <= 0:
        pytest.fail("GPU test selected but no HIP device is visible (libmcrt has no CPU fallback)")
    return 0
