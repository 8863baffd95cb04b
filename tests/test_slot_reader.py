"""CPU tier: SlotReader (bonsai_amd/csrc/host/bns_slot_reader.hpp), the one loop that reads the inputs of the device-text pipelines into
page-locked slots -- alone, on small files and pageable memory, in the shapes where such a loop goes wrong.  One run of
bin/bns_slot_check (tests/helpers/slot_reader_harness.cpp) per scenario; the program ends itself after 20 s, so a lost wake-up fails."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHECK = os.path.join(ROOT, "bonsai_amd", "bin", "bns_slot_check")


@pytest.fixture(scope="module")
def check():
    from bonsai_amd.build import build_device_library
    build_device_library()
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "bonsai_amd", "csrc", "host")], check=True)
    return CHECK


def run(check, scenario, tmp_path):
    r = subprocess.run([check, scenario, str(tmp_path)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=60)
    facts = dict(kv.split("=", 1) for line in r.stdout.splitlines() for kv in ([line] if line.startswith("error=") else line.split()))
    print(r.stdout, r.stderr)
    assert r.returncode >= 0, "killed by signal %d (14: a wake-up was lost)" % -r.returncode
    return r.returncode, facts


def test_every_byte_in_order_within_the_cap(check, tmp_path):
    # 1,000,003 bytes in slots of 64 KiB + 4 KiB of overlap, 4 KiB pieces, 4 readers, at most 3 slots
    rc, f = run(check, "in_order", tmp_path)
    assert int(f["slots"]) == 16 and int(f["good"]) == 16      # every slot arrived, each equal to the file's bytes at its offset
    assert int(f["made"]) <= 3
    assert f["cancelled"] == "0" and rc == 0                    # (the readers left by themselves: the program joined them without a cancel)


def test_two_spans_from_two_files(check, tmp_path):
    rc, f = run(check, "two_files", tmp_path)
    assert int(f["slots"]) == 5 and int(f["good"]) == 5 and int(f["made"]) <= 3
    assert int(f["empty_second"]) == 3                          # the shorter second file: slots 2, 3, 4 read nothing of it
    assert int(f["empty_slots"]) == 1 and int(f["empty_good"]) == 1     # an empty input is one slot, loaded at once
    assert rc == 0


def test_cancel_while_blocked(check, tmp_path):
    rc, f = run(check, "cancel_blocked", tmp_path)
    assert f["joined"] == "1" and int(f["made"]) == 3 and int(f["opened"]) == 3 and rc == 0


def test_short_read(check, tmp_path):
    rc, f = run(check, "short_read", tmp_path)
    assert f["error"] == "short read in test file"
    assert f["cancelled"] == "1" and f["woken"] == "1" and int(f["good"]) < 4 and rc == 0


def test_stop_opening(check, tmp_path):
    rc, f = run(check, "stop_opening", tmp_path)
    assert int(f["opened"]) == int(f["opened_at_stop"]) < int(f["slots"])      # no further slot after the stop
    assert int(f["good"]) == int(f["opened"])                   # the ones that were loading finished, intact
    assert f["cancelled"] == "0" and rc == 0
