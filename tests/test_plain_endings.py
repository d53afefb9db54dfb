"""Repetition, the 75-move rule, draws by material and the position key held to a plain restatement (tests/plainendings.py).  CPU only.

Until here the rules that end a game or count a repetition had builder-authored tests only: the oracle (oracle/oc_chess.c), the host
mirror (csrc/sz_host.cpp) and the device share an author, and the last two share sz_chess.h (sz_hash_key, sz_finish_meta, the irrev
flag, sz_insufficient_side).  tests/plainendings.py states those rules a second time, from the rules as python-chess documents them and
in another shape (whole-game identity tuples, no hash, no window).  Here
  (1) after EVERY ply of every line of tests/ending_lines.py (filler included) and of every random game, the host mirror and the oracle
      each equal the plain statement on the legal moves, get_value_and_terminated(), the repetition planes 12 and 13 of the newest
      history step, the repetition count the mirror keeps (capped at 4), is_repetition(2..5) of the oracle, and the halfmove clock;
  (2) over all those positions together: equal plain identity <=> equal key word of the host mirror's record, exactly.  One direction
      catches a key that forgets rights, turn or the legal en-passant square, or that includes the clock or an illegal en-passant
      square; the other catches collisions;
  (3) the plain full-history repetition count equals the count over the plies since the last pawn move, capture or loss of a right, the
      argument of plainendings' docstring;
  (4) every mate witness of the material table is a checkmate by plainrules, holds exactly its signature's men, and the witnesses are
      exactly the signatures the table calls sufficient.  That anchors the "sufficient" direction; the "insufficient" one is a restatement;
  (5) the checks have teeth: five wrong clauses, each put into a COPY of the plain statement, each make named lines fail.
No tolerance anywhere, nothing skipped.

Reached by the committed seed (printed by the tests; the module takes 31 s, 14 s of it the random games):
  405 random games from 15 starts, 32,375 positions; ended by mate 10, stalemate 34, material 257, 75 moves 31, fivefold 60, cut at 300
  plies 13; 416 positions with two or more earlier equal ones; 18 games longer than 256 plies (the device's ring);
  80 lines with their histories and filler, 4,837 positions;
  key comparison: 37,212 positions, 30,193 distinct identities = 30,193 distinct keys; window argument: 37,212 positions, 4,028 of them
  with a repetition count above 0.
"""
import numpy as np
import pytest

from sigma_zero_amd import _native as N
from oracle import oracle as O
import ending_lines as L
import plainendings as E
import plainrules as P

_RECORDS = {}                       # (what) -> [(identity, key, tag)], filled by the two walking tests and read by the key test


def oracle_game(fen, chess960):
    return O.ChessTensor() if fen is None else O.ChessTensor.from_fen(fen, chess960=chess960)


def compare_game(tag, fen, chess960, game, records=None):
    """the plain Game `game`, ply by ply, against the host mirror and the oracle: (1) of the module docstring"""
    ct, oct_ = L.host_game(fen, chess960), oracle_game(fen, chess960)
    lib = N.lib()
    planes = np.zeros((N.SZ_PLANES, 64), np.uint8)
    for ply in range(len(game) + 1):
        where = "%s, ply %d" % (tag, ply)
        pos, legal = game.pos[ply], game.legal[ply]
        want_moves = {L.host_spelling(pos, m, chess960) for m in legal}
        acts = L.host_actions(ct)
        assert set(acts) == want_moves, "%s: host mirror: legal moves: only the mirror %s, only the plain statement %s" % (
            where, sorted(set(acts) - want_moves), sorted(want_moves - set(acts)))
        ob = oct_.board
        got = {m.key() for m in ob.legal_moves()}
        assert got == want_moves, "%s: oracle: legal moves: only the oracle %s, only the plain statement %s" % (
            where, sorted(got - want_moves), sorted(want_moves - got))
        want = game.value_and_terminated(ply)
        assert ct.get_value_and_terminated() == want, "%s: host mirror says %s, the plain statement %s (%s)" % (
            where, ct.get_value_and_terminated(), want, game.outcome(ply))
        assert oct_.get_value_and_terminated() == want, "%s: oracle says %s, the plain statement %s (%s)" % (
            where, oct_.get_value_and_terminated(), want, game.outcome(ply))
        count = game.repetition_count(ply)
        rep = [game.is_repetition(n, ply) for n in (2, 3)]
        lib.szh_planes(ct._g, planes.ctypes.data)
        for name, pl in (("host mirror", planes), ("oracle", oct_.get_representation().reshape(N.SZ_PLANES, 64))):
            for k in (0, 1):
                assert pl[12 + k].all() == pl[12 + k].any() == rep[k], "%s: %s: repetition plane %d, the plain statement counts %d" % (
                    where, name, 12 + k, count)
        st = ct.board._st()
        assert st[7] == min(count, 4), "%s: host mirror counts %d repetitions, the plain statement %d" % (where, st[7], count)
        for n in (2, 3, 4, 5):
            assert ob.is_repetition(n) == game.is_repetition(n, ply), "%s: oracle is_repetition(%d)" % (where, n)
        assert st[2] == game.clock[ply] == ob.halfmove_clock, "%s: halfmove clock: host mirror %d, oracle %d, plain statement %d" % (
            where, st[2], ob.halfmove_clock, game.clock[ply])
        assert st[0] == int(pos.white) and st[1] == ob.ply
        if records is not None:
            records.append((game.ids[ply], ct.board.bitboards()[8], where))
        if ply < len(game):
            m = L.host_spelling(pos, game.moves[ply], chess960)
            ct.push_action(acts[m])
            oct_.move_piece(O.Move(*m))


def compare_line(line, rules=E.RULES, records=None):
    b = L.build(line, 40, rules)
    compare_game(b.name, b.fen, b.chess960, b.game, records)
    return b


def test_lines_against_host_mirror_and_oracle():
    """(1) on the 80 lines: 4,837 positions, histories and filler included"""
    rec = _RECORDS["lines"] = []
    built = [compare_line(line, records=rec) for line in L.LINES]
    print("%d lines, %d positions" % (len(built), len(rec)))
    assert {b.kind for b in built} == set(L.KINDS)
    assert max(b.scripted for b in built if b.over_depth == b.scripted) >= 16      # an ending as deep as 16 plies below the root


def test_random_games_against_host_mirror_and_oracle():
    """(1) on the random games, after ending_lines.COVERAGE was asserted on the plain statement alone.  Reached: 405 games, 32,375
    positions; mate 10, stalemate 34, material 257, 75 moves 31, fivefold 60; 416 positions with a repetition count >= 2; 18 games
    longer than 256 plies."""
    games = L.random_games()
    got = L.check_coverage(games)
    print(got)
    rec = _RECORDS["games"] = []
    for k, (name, fen, c960, g) in enumerate(games):
        compare_game("random game %d from %s" % (k, name), fen, c960, g, rec)
    assert len(rec) == got["positions"] >= 20000


def test_equal_identity_is_equal_key():
    """(2): over the positions of both walks above; runs them if they have not run"""
    if "lines" not in _RECORDS:
        test_lines_against_host_mirror_and_oracle()
    if "games" not in _RECORDS:
        test_random_games_against_host_mirror_and_oracle()
    rec = _RECORDS["lines"] + _RECORDS["games"]
    key_of, id_of = {}, {}
    for ident, key, where in rec:
        k, w = key_of.setdefault(ident, (key, where))
        assert k == key, "one position, two keys: %s has %#018x and %s has %#018x" % (w, k, where, key)
        i, w = id_of.setdefault(key, (ident, where))
        assert i == ident, "two positions, one key %#018x: %s and %s" % (key, w, where)
    print("%d positions, %d distinct identities, %d distinct keys" % (len(rec), len(key_of), len(id_of)))
    assert len(key_of) == len(id_of) and len(rec) >= 20000
    repeated = len(rec) - len(key_of)
    assert repeated >= 1000                                             # the first direction was asked often


def test_full_history_count_equals_the_windowed_count():
    """(3)"""
    n = differ = 0
    games = [g for _, _, _, g in L.random_games()] + [L.build(line, 40).game for line in L.LINES]
    for g in games:
        for ply in range(len(g) + 1):
            full, window = g.repetition_count(ply), g.windowed_count(ply)
            assert full == window, "ply %d: %d earlier equal positions in the whole game, %d since the last irreversible move" % (ply, full, window)
            n += 1
            differ += full > 0
    print("%d positions, %d with a count above 0" % (n, differ))
    assert n >= 20000 and differ >= 1000


def test_mate_witnesses_anchor_the_sufficient_side_of_the_material_table():
    """(4)"""
    sufficient = {s for s in E.pawnless_signatures(4) if E.table_says_sufficient(s)}
    assert set(E.MATE_WITNESSES) == sufficient and len(sufficient) == 25
    for sig, fen in E.MATE_WITNESSES.items():
        pos = P.from_fen(fen)
        assert not pos.white and P.is_checkmate(pos), "%s: %s is no checkmate" % (sig, fen)
        assert not P.in_check(pos, True), "%s: %s: both kings are attacked" % (sig, fen)
        assert E.fold(E.signature(pos.board, True)) == sig, "%s: %s holds other men" % (sig, fen)
        assert not E.RULES.insufficient_side(pos.board, True) and not E.RULES.insufficient(pos.board)
    # the signatures of at most four men the table calls insufficient for a side: a restatement, listed so that a change shows
    insufficient = sorted(s for s in E.pawnless_signatures(4) if not E.table_says_sufficient(s))
    assert insufficient == [("", ""), ("", "D"), ("", "DD"), ("", "DL"), ("", "DN"), ("", "DQ"), ("", "DR"), ("", "N"), ("", "NN"), ("", "NQ"),
                            ("", "NR"), ("", "Q"), ("", "QQ"), ("", "QR"), ("", "R"), ("", "RR"), ("D", ""), ("D", "D"), ("D", "Q"), ("D", "R"),
                            ("DD", ""), ("N", ""), ("N", "Q")]


# ------------------------------------------------------------------------------------------------ (5) teeth
class _IgnoresRights(E.Rules):
    def identity(self, pos, legal):
        return (tuple(pos.board), pos.white, pos.ep if self.legal_en_passant(pos, legal) else None)


class _KeepsIllegalEnPassant(E.Rules):
    def identity(self, pos, legal):
        return (tuple(pos.board), pos.white, frozenset(pos.rights), pos.ep)


class _Clock149(E.Rules):
    CLOCK_LIMIT = 149


class _ClockBeforeMate(E.Rules):
    def outcome(self, pos, legal, clock, count):
        if clock >= self.CLOCK_LIMIT:
            return (E.CLOCK, 0)
        return E.Rules.outcome(self, pos, legal, clock, count)


class _OwnBishopsOnly(E.Rules):
    def insufficient_side(self, board, white):
        if sorted(c.upper() for c in board if c != "." and c.isupper() == white).count("B") and not any(
                c.upper() in "PRQN" for c in board if c != "." and c.isupper() == white):
            colours = {E.square_is_dark(s) for s in range(64) if board[s] == ("B" if white else "b")}
            return len(colours) == 1 and not any(c in "PpNn" for c in board)
        return E.Rules.insufficient_side(self, board, white)


TEETH = [
    (_IgnoresRights, "identity:king_out_and_back_loses_the_rights"),
    (_KeepsIllegalEnPassant, "identity:double_push_capturer_is_pinned"),
    (_Clock149, "clock:draw_at_depth_07"),
    (_ClockBeforeMate, "mate150:depth_5"),
    (_OwnBishopsOnly, "material_goes_on:opposite_bishops_at_depth_5"),
]


@pytest.mark.parametrize("rules,named", TEETH, ids=[t[0].__name__.strip("_") for t in TEETH])
def test_a_wrong_clause_in_a_copy_of_the_plain_statement_fails_named_lines(rules, named):
    """Symmetric injection: the shipped code is untouched, the wrong clause sits in a copy of the plain statement.  Every line is built
    (its claim) and compared with the host mirror and the oracle as in (1); the lines that fail are collected by name."""
    failed = {}
    for line in L.LINES:
        try:
            compare_line(line, rules())
        except AssertionError as e:
            failed[line[0]] = str(e).splitlines()[0]
    print("%s: %d of %d lines fail, e.g. %s" % (rules.__name__, len(failed), len(L.LINES), failed.get(named)))
    assert named in failed, "%s goes unnoticed by %s" % (rules.__name__, named)
    # and by the comparison with the other two statements alone, the claims aside: on the named line's own game
    b = L.build([l for l in L.LINES if l[0] == named][0], 40)
    with pytest.raises(AssertionError):
        compare_game(named, b.fen, b.chess960, b.game.retold(rules()))
