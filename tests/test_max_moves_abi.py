"""The move limit of the device environments (config.max_moves inside the environment kernels), the parts that need no
GPU: the library exports mzenv_set_max_moves / mzenv_game_moves, the Python binding declares them with the argument
lists of include/mzenv.h, the header documents them, their argument checks run without a device, and the history filer
files a game of exactly max_moves plies into rows of max_moves + 1."""
import ctypes
import importlib
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("mzenv_set_max_moves", "mzenv_game_moves")


@pytest.fixture(scope="module")
def native(pkg):
    importlib.import_module("muzero-hypermodel_amd.build").build_native()
    return importlib.import_module("muzero-hypermodel_amd._native")


def header():
    return open(os.path.join(ROOT, "include", "mzenv.h")).read()


def declared_arguments(name):
    """ctypes argument list of `name` as include/mzenv.h declares it: pointers travel as void pointers."""
    code = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    found = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, code)
    assert found, f"{name} is not declared in include/mzenv.h"
    args = []
    for arg in found.group(1).split(","):
        if "*" in arg:
            args.append(ctypes.c_void_p)
        else:
            assert arg.split()[0] == "int32_t", arg
            args.append(ctypes.c_int32)
    return args


def test_library_exports_and_binding_declares_the_move_limit(native):
    lib = native.load()
    for name in NEW:
        assert hasattr(lib, name), f"{name} is not exported by libmzmcts.so"
        restype, argtypes = native.PROTOTYPES[name]
        assert restype is ctypes.c_int and list(argtypes) == declared_arguments(name), name
        assert list(getattr(lib, name).argtypes) == declared_arguments(name)


def test_header_documents_the_move_limit():
    text = header()
    section = text[text.index("move limit"):]
    assert all(name in section for name in NEW)
    doc = " ".join(section.split()).lower().replace("* ", "")
    # the sentence that matters to callers, the default, the counter's rules and what set_boards does to it
    assert 'done means "the game is over", not "the position is terminal"' in doc
    assert "0 (the value at create) = no limit" in doc and "negative: error" in doc
    assert "opponent's plies too" in doc and "does not count" in doc
    assert "dev i32[e]" in doc and "asynchronous and allocation-free" in doc
    boards = text[text.index("Put every env of a board game"):text.index("int mzenv_set_boards")]
    assert "number of stones" in " ".join(boards.split())


def test_move_limit_argument_checks_need_no_device(native):
    """A negative limit is refused before the handle is looked at; null handles and null outputs are errors."""
    lib = native.load()
    assert lib.mzenv_set_max_moves(None, -1) == -1
    assert b"number of plies" in lib.mzenv_last_error(None)
    assert lib.mzenv_set_max_moves(None, 5) == -1
    assert b"null handle" in lib.mzenv_last_error(None)
    assert lib.mzenv_game_moves(None, None, None) == -1
    assert b"mzenv_game_moves" in lib.mzenv_last_error(None)


def test_history_filer_files_games_of_exactly_max_moves(pkg):
    """Rows of max_moves + 1 (what DeviceSelfPlay gives its filer) take games that the limit ends at ply max_moves --
    inside a batch, on its last move and across two batches -- and every game comes out whole."""
    sp = importlib.import_module("muzero-hypermodel_amd.self_play")
    E, A, S, limit = 3, 2, 10, 5
    obs_shape = (1, 1, 4)
    rs = np.random.RandomState(11)
    filer = sp.HistoryFiler(E, limit + 1, obs_shape, A)
    first = rs.randn(E, *obs_shape).astype(np.float32)
    filer.begin(first, np.zeros(E, np.int32))
    legal = np.tile(np.arange(A, dtype=np.int32), (E, 1))
    num_legal = np.full(E, A, np.int32)
    ply = np.zeros(E, np.int64)
    games = {e: [] for e in range(E)}
    want = {e: [[]] for e in range(E)}
    for M in (3, 2, 7, 3):                                     # 15 plies: three games of 5 per env
        out = dict(actions=rs.randint(0, A, (M, E)).astype(np.int32), visits=rs.randint(0, S, (M, E, A)).astype(np.int32),
                   root_value_sum=rs.randn(M, E), moves_done=np.full(E, M, np.int32))
        done = np.zeros((M, E), np.uint8)
        for m in range(M):
            ply += 1
            done[m] = ply % limit == 0
            for e in range(E):
                want[e][-1].append(int(out["actions"][m, e]))
                if done[m, e]:
                    want[e].append([])
        rewards = np.ones((M, E), np.float32)
        obs_after = rs.randn(M, E, *obs_shape).astype(np.float32)
        obs_next = rs.randn(M, E, *obs_shape).astype(np.float32)
        batch = filer.file(out, legal, num_legal, S, rewards, done, obs_after, obs_next)
        for i in range(0 if batch is None else len(batch)):
            games[int(batch.env_index[i])].append(batch.history(i))
        assert (filer.lengths() == ply % limit).all()
    for e in range(E):
        assert len(games[e]) == 3
        for gh, actions in zip(games[e], want[e]):
            assert gh.action_history == [0] + actions and len(gh.action_history) == limit + 1
            assert len(gh.child_visits) == len(gh.root_values) == limit and gh.reward_history == [0.0] + [1.0] * limit
