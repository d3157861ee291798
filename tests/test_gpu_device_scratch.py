"""GPU: the holder of per-call device memory (csrc/device_scratch.hpp) through its self-test hook, which launches no kernel.
Blocks land on the holder's device whatever device the calling thread has current, never have less than 16 bytes of room, and a
refused request leaves a null pointer and the blocks already held alone."""
import pytest

pytestmark = pytest.mark.gpu


def check_holder(home, current):
    from usearch_amd import index as ua
    report = ua.test_device_scratch(home, current)
    pointers = report["pointers"]
    assert all(pointers) and len(set(pointers)) == 3, pointers
    # blocks asked for 0, 1 and 4096 bytes: the 16-byte floor, then what was asked
    assert report["room"][0] >= 16 and report["room"][1] >= 16 and report["room"][2] >= 4096, report["room"]
    # 2^60 bytes are refused, the out-pointer comes back null, and the three blocks are still there, on the home device
    assert report["refused"] != 0 and report["refused_pointer"] == 0, report
    assert report["devices"] == [home] * 3, report["devices"]


def test_blocks_live_on_the_current_device_when_it_is_home():
    check_holder(home=0, current=0)


def test_blocks_live_on_home_when_another_device_is_current():
    import usearch_amd
    if usearch_amd.device_count() < 2:
        pytest.skip("needs two devices")
    check_holder(home=0, current=1)
    check_holder(home=1, current=0)
