"""The ABI version the tests pin, stated once.  A plain module (no test in it): bump RN_VERSION here together with the
`#define RN_VERSION` of include/rendernet_hip.h; tests/test_host_cpu.py holds it against rn_version() of the built library."""
import re

RN_VERSION = 193


def states_version(header_text):
    """The header text defines RN_VERSION as the pinned value."""
    return re.search(r"#define\s+RN_VERSION\s+%d\b" % RN_VERSION, header_text) is not None
