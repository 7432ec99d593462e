// paired_moves.h -- the slot rule of a paired move (include/mzenv.h mzenv_advance_paired): MuZero's ply and the scripted
// opponent's replies in ONE launch, so that no env of an evaluation batch sits a search out.  The environment kernels
// (env_kernels.hip, every form) and a CPU check (tests/paired_moves_check.cpp) compile this same text.
//
// A move of one env is kPairedSlots ply slots, run in order:
//   slot 0      MuZero's ply: played only if MuZero is to move and the incoming action is >= 0; otherwise empty
//   slot 1, 2   an opponent's ply each: played only while the opponent is to move.  Slot 1 is the reply -- or the opening
//               of the next game when MuZero's own ply ended the game and MuZero plays second; slot 2 can only be that
//               opening after a reply that ended the game.
// A ply is what a single-ply launch does for the env: step, observation of the position reached, reset if the game is
// over (by its rules or by the move limit).  After the three slots MuZero is to move in every env -- unless the move
// limit is 1 and MuZero plays second (opening, limit, reset, opening, ...), which mzenv_advance_paired refuses.
//
// The rule knows no game: `Ops` plays the plies.  Every slot is visited with a flag instead of being skipped, so that a
// form whose ply is collective (Gomoku's wavefront per env, with workgroup barriers inside) runs uniform control flow.
//   bool Ops::opponent_to_move()           the side to move now is the scripted opponent's
//   void Ops::slot(int s, bool play, int a) play == true: one ply into slot s (a >= 0: that action; a < 0: the opponent
//                                           chooses from the env's stream); play == false: slot s is empty
#pragma once

#ifndef MZ_HD
#ifdef __HIPCC__
#define MZ_HD __host__ __device__
#else
#define MZ_HD
#endif
#endif

namespace mz {

constexpr int kPairedSlots = 3;

template <class Ops>
MZ_HD inline void paired_move(Ops& ops, int action) {
    for (int s = 0; s < kPairedSlots; ++s) {
        const bool opponent = ops.opponent_to_move();
        const bool play = s == 0 ? (!opponent && action >= 0) : opponent;
        ops.slot(s, play, s == 0 ? action : -1);
    }
}

}  // namespace mz
