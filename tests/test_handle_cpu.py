"""plslam_amd._lib.Handle, the life cycle every library object shares, on a stub library that records its calls (nothing of
the real library is freed here), and PinnedArray's failure path.  No GPU needed."""
import gc
import inspect
import weakref

import pytest

import plslam_amd
from plslam_amd import _lib, lc_fuse, local_map, map_insert, map_lists
from plslam_amd._lib import Handle


class StubLib:
    def __init__(self, fail=False):
        self.calls, self.fail = [], fail

    def plslam_thing_destroy(self, h):
        self.calls.append(("plslam_thing_destroy", h))
        if self.fail:
            raise RuntimeError("destroy failed")


class StubContext:
    def __init__(self, lib):
        self._L, self.handle = lib, 0x1000


class Thing(Handle):
    def __init__(self, ctx, h):
        self._open(ctx, "plslam_thing_destroy", h)


def test_close_destroys_once_with_the_handle():
    lib = StubLib()
    t = Thing(StubContext(lib), 0xbeef)
    assert t.handle == 0xbeef
    t.close()
    assert lib.calls == [("plslam_thing_destroy", 0xbeef)] and t.handle is None
    t.close()
    t.__del__()
    del t
    gc.collect()
    assert lib.calls == [("plslam_thing_destroy", 0xbeef)]


def test_del_destroys_a_handle_left_open():
    lib = StubLib()
    t = Thing(StubContext(lib), 0xbeef)
    del t
    gc.collect()
    assert lib.calls == [("plslam_thing_destroy", 0xbeef)]


def test_a_null_handle_is_not_destroyed():
    lib = StubLib()
    for null in (None, 0, _lib.C.c_void_p()):
        Thing(StubContext(lib), null).close()
    Thing.__new__(Thing).close()       # (an object whose create call raised: nothing was opened)
    assert lib.calls == []


def test_after_the_context_closed_the_handle_is_only_dropped():
    lib = StubLib()
    ctx = StubContext(lib)
    t = Thing(ctx, 0xbeef)
    ctx.handle = None
    t.close()
    assert lib.calls == [] and t.handle is None
    ctx.handle = 0x1000                # (even a context that came back: the handle is gone)
    t.close()
    assert lib.calls == []


def test_an_exception_of_the_destroy_stays_inside_del():
    lib = StubLib(fail=True)
    t = Thing(StubContext(lib), 0xbeef)
    t.__del__()
    assert lib.calls == [("plslam_thing_destroy", 0xbeef)] and t.handle is None
    with pytest.raises(RuntimeError):
        Thing(StubContext(lib), 0xcafe).close()


def test_a_live_handle_keeps_its_context_alive():
    lib = StubLib()
    ctx = StubContext(lib)
    ref = weakref.ref(ctx)
    t = Thing(ctx, 0xbeef)
    del ctx
    gc.collect()
    assert ref() is not None
    t.close()
    assert lib.calls == [("plslam_thing_destroy", 0xbeef)]     # (the context was still open: destroyed, not dropped)
    del t
    gc.collect()
    assert ref() is None


def test_a_context_is_its_own_context_without_a_reference_cycle():
    lib = StubLib()

    class Ctx(Handle):
        def __init__(self):
            self._L = lib
            self._open(self, "plslam_thing_destroy", 0x1000)

    c = Ctx()
    ref = weakref.ref(c)
    gc.disable()
    try:
        del c                          # freed by its reference count, as a context always was
        assert ref() is None and lib.calls == [("plslam_thing_destroy", 0x1000)]
    finally:
        gc.enable()


HANDLE_CLASSES = ("MatchPlan", "GridPlan", "MatchPipeline", "LbaPlan", "GbaPlan", "PgoPlan", "LcBatch", "BowVocabulary", "BowDatabase")


def test_every_handle_class_closes_through_handle():
    classes = [getattr(plslam_amd.capi, n) for n in HANDLE_CLASSES] + [plslam_amd.Context, local_map.LocalMap, map_insert.MapInsert,
                                                                       lc_fuse.LcFuse]
    for cls in classes:
        assert issubclass(cls, Handle), cls
        assert "close" not in vars(cls) and "__del__" not in vars(cls) and "handle" not in vars(cls), cls
    # map_lists.MapLists owns nothing (its three calls run on the handles of MapInsert / LcFuse): no other class of the package
    # has a close or a __del__ of its own but PinnedArray, which frees a pointer and needs no context
    own = set()
    for mod in (plslam_amd.capi, _lib, local_map, map_insert, lc_fuse, map_lists):
        for name, cls in inspect.getmembers(mod, inspect.isclass):
            if cls.__module__.startswith("plslam_amd") and ({"close", "__del__"} & set(vars(cls))):
                own.add(name)
    assert own == {"Handle", "PinnedArray"}


def test_pinned_array_reports_no_memory(monkeypatch):
    L = plslam_amd.load()
    monkeypatch.setattr(L, "plslam_pinned_alloc", lambda nbytes: 0)

    class Ctx:
        _L = L

    with pytest.raises(plslam_amd.PlslamError) as e:
        plslam_amd.PinnedArray(Ctx(), (16,), "uint8")
    assert e.value.code == plslam_amd.capi.ENOMEM and "plslam_pinned_alloc" in str(e.value)
