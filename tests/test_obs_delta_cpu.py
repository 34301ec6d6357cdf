"""CPU-side pieces of the delta obs writer (no GPU): the destination table's LRU / forget logic
(csrc/obs_dest.h, host-only C++, compiled into a stand-alone program) and VecGridEnv's destination
guard against a stub library."""
import os
import subprocess

import torch

from marlnav import _lib
from marlnav import vec_env as V

TABLE_PROGRAM = r"""
#include <cassert>
#include <cstdio>
#include "obs_dest.h"
int main() {
    using gwdest::SLOTS;
    gwdest::Table t;
    char mem[64];
    auto P = [&](int i) { return (const void *)(mem + i); };
    assert(t.find(P(0), 0) == -1 && t.count() == 0);
    // a full write claims a slot; the same pointer in the other dtype is unknown and replaces it
    const int a = t.claim(P(0), 0);
    assert(t.find(P(0), 0) == a && t.find(P(0), 1) == -1 && t.find(P(1), 0) == -1);
    assert(t.claim(P(0), 1) == a && t.find(P(0), 0) == -1 && t.find(P(0), 1) == a && t.count() == 1);
    assert(t.forget(P(0)) == 1 && t.find(P(0), 1) == -1 && t.forget(P(0)) == 0);
    // fill the table: every pointer keeps its own slot
    int s[SLOTS + 2];
    for (int i = 0; i < SLOTS; ++i) s[i] = t.claim(P(i), 0);
    for (int i = 0; i < SLOTS; ++i)
        for (int j = 0; j < i; ++j) assert(s[i] != s[j]);
    assert(t.count() == SLOTS);
    // use all but pointer 3 again: the next new pointer evicts 3 (least recently used) and only 3
    for (int i = 0; i < SLOTS; ++i)
        if (i != 3) assert(t.find(P(i), 0) == s[i]);
    assert(t.claim(P(SLOTS), 0) == s[3] && t.find(P(3), 0) == -1 && t.count() == SLOTS);
    for (int i = 0; i < SLOTS; ++i)
        if (i != 3) assert(t.find(P(i), 0) == s[i]);
    // a freed slot is taken before anything is evicted
    assert(t.forget(P(5)) == 1 && t.claim(P(SLOTS + 1), 0) == s[5] && t.find(P(0), 0) == s[0]);
    // round robin over SLOTS + 1 pointers never finds one (each comes back after its eviction)
    t.forget(nullptr);
    assert(t.count() == 0);
    for (int r = 0; r < 3 * (SLOTS + 1); ++r) {
        assert(t.find(P(r % (SLOTS + 1)), 0) == -1);
        t.claim(P(r % (SLOTS + 1)), 0);
    }
    assert(t.forget(nullptr) == SLOTS && t.count() == 0);
    std::puts("ok");
    return 0;
}
"""


def test_destination_table_lru_and_forget(tmp_path):
    src = tmp_path / "table.cpp"
    src.write_text(TABLE_PROGRAM)
    exe = tmp_path / "table"
    subprocess.run(["g++", "-std=c++17", "-O1", "-fsanitize=address,undefined", f"-I{_lib.CSRC}", str(src), "-o",
                    str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stderr


def test_header_and_binding_agree_on_the_table_size():
    text = open(os.path.join(_lib.INCLUDE, "gridenv.h")).read()
    assert f"#define GW_OBS_DESTS {_lib.GW_OBS_DESTS}" in text
    assert f"constexpr int SLOTS = {_lib.GW_OBS_DESTS};" in open(os.path.join(_lib.CSRC, "obs_dest.h")).read()


class StubLib:
    def __init__(self):
        self.forgot = []

    def gw_obs_dest_forget(self, handle, ptr):
        self.forgot.append(ptr)
        return 0


def _guarded():
    env = object.__new__(V.VecGridEnv)
    env.lib, env.handle, env._dest_guard, env._uid, env._closed = StubLib(), None, {}, next(V._UIDS), True
    return env


def test_guard_trusts_only_what_it_can_check():
    env = _guarded()
    ring = torch.zeros(5, 2, 4, 3, 3)
    a = ring[0]
    env._guard_dest(a)
    env._guard_dest(a)
    env._guard_dest(ring[0])  # another view object of the same bytes
    assert env.lib.forgot == []
    a.fill_(1.0)  # a write torch sees
    env._guard_dest(a)
    assert env.lib.forgot == [a.data_ptr()]
    env._guard_dest(ring[1])
    env._guard_dest(ring[1])
    ring[3].copy_(ring[2])  # into ANOTHER slot: views share the version counter
    env._guard_dest(ring[0])
    env._guard_dest(ring[1])
    assert env.lib.forgot == [a.data_ptr(), ring[0].data_ptr(), ring[1].data_ptr()]
    env._guard_dest(ring[0])
    assert len(env.lib.forgot) == 3
    # the same address, another size
    env._guard_dest(ring[0].reshape(-1)[:8])
    assert env.lib.forgot[3:] == [ring[0].data_ptr()]


def test_guard_holds_the_tensor_and_bounds_its_table():
    env = _guarded()
    t = torch.zeros(16)
    ptr = t.data_ptr()
    env._guard_dest(t)
    assert env._dest_guard[ptr][0] is t  # a reference: the allocator cannot recycle the address
    bufs = [torch.zeros(16) for _ in range(_lib.GW_OBS_DESTS)]
    for b in bufs:
        env._guard_dest(b)
    assert len(env._dest_guard) == _lib.GW_OBS_DESTS and env.lib.forgot == [ptr]  # the oldest was dropped
    # least recently used, as the library's table: a hit refreshes a destination's place
    env._guard_dest(bufs[0])
    extra = torch.zeros(16)
    env._guard_dest(extra)
    assert env.lib.forgot == [ptr, bufs[1].data_ptr()] and bufs[0].data_ptr() in env._dest_guard
    env.obs_dest_forget(None)
    assert env._dest_guard == {} and env.lib.forgot[-1] is None


def test_queued_lazy_destination_is_vetted_again():
    """Lazy async obs: the destination of the writer still queued is checked again before the call
    that launches it (the next step, a fence, a reset)."""
    env = _guarded()
    env.obs_delta, env._queued_dest = True, None
    t = torch.zeros(16)
    env._guard_dest(t)
    env._queued_dest = t
    env._guard_queued()
    assert env.lib.forgot == []
    t.fill_(1.0)
    env._guard_queued()
    assert env.lib.forgot == [t.data_ptr()]
    env._guard_queued()  # vetted and recorded again: nothing more to forget
    assert env.lib.forgot == [t.data_ptr()]


def test_another_env_writing_the_buffer_is_noticed():
    a, b = _guarded(), _guarded()
    t = torch.zeros(16)
    a._guard_dest(t)
    a._guard_dest(t)
    b._guard_dest(t)  # torch's version counter cannot see either env's kernel
    assert a.lib.forgot == []
    a._guard_dest(t)
    assert a.lib.forgot == [t.data_ptr()]
    b._guard_dest(t)
    assert b.lib.forgot == [t.data_ptr()]
