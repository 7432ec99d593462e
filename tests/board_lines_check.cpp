// Host-side check of csrc/board_rules.h (the text the environment kernels compile), row by row: where
// board_rules_check.cpp counts mismatches against HostStream, this program REPORTS what the header says and leaves the
// judging to the test, which holds the reports to fixture G24 (recorded from the reference).  Rows read from stdin:
//     P game(1|2) player(+1|-1) action cells x stone
//         the stone is placed as the environment kernels place it (tic-tac-toe: the cell; connect four: the lowest empty
//         cell of the column) and one line is written:   P won(+1) won(-1) n_legal legal...
//     X game(1|2) player(+1|-1) seed cells x stone
//         the scripted expert moves on a stream seeded `seed`, then the random opponent on a fresh one:
//             X expert_move words stream_position stream_equals_hoststream(0|1) random_move random_words
// Built and run by tests/test_board_rules_cpu.py, once plainly and once with -fsanitize=address,undefined:
//     g++ -O2 -std=c++17 -ffp-contract=off board_lines_check.cpp -lm
#include <cstdio>
#include <cstring>

#include "board_rules.h"

static bool read_board(int cells, int8_t* board) {
    for (int i = 0; i < cells; ++i) {
        int v;
        if (std::scanf("%d", &v) != 1 || v < -1 || v > 1) return false;
        board[i] = static_cast<int8_t>(v);
    }
    return true;
}

int main() {
    char mode[4];
    int game, player;
    long rows = 0;
    while (std::scanf("%3s %d %d", mode, &game, &player) == 3) {
        if ((game != 1 && game != 2) || (player != 1 && player != -1)) return 2;
        const int cells = game == 1 ? 9 : 42;
        int8_t board[42];
        if (mode[0] == 'P') {
            int action;
            if (std::scanf("%d", &action) != 1 || !read_board(cells, board)) return 2;
            if (game == 1) {
                if (action < 0 || action >= 9 || board[action] != 0) return 3;
                board[action] = static_cast<int8_t>(player);
            } else {
                if (action < 0 || action >= 7 || board[35 + action] != 0) return 3;
                for (int r = 0; r < 6; ++r)
                    if (board[r * 7 + action] == 0) {
                        board[r * 7 + action] = static_cast<int8_t>(player);
                        break;
                    }
            }
            int32_t legal[9];
            const int n = game == 1 ? mz::ttt_legal(board, legal) : mz::c4_legal(board, legal);
            const bool plus = game == 1 ? mz::ttt_winner(board, 1) : mz::c4_winner(board, 1);
            const bool minus = game == 1 ? mz::ttt_winner(board, -1) : mz::c4_winner(board, -1);
            std::printf("P %d %d %d", plus ? 1 : 0, minus ? 1 : 0, n);
            for (int i = 0; i < n; ++i) std::printf(" %d", legal[i]);
            std::printf("\n");
        } else if (mode[0] == 'X') {
            unsigned seed;
            if (std::scanf("%u", &seed) != 1 || !read_board(cells, board)) return 2;
            int32_t legal[9];
            const int n = game == 1 ? mz::ttt_legal(board, legal) : mz::c4_legal(board, legal);
            if (n == 0) return 3;
            int moves[2];
            uint32_t drawn[2];
            int32_t expert_pos = 0;
            bool same = true;
            for (int kind = mz::kOpponentExpert; kind <= mz::kOpponentRandom; ++kind) {
                mz::HostStream host;
                host.seed(seed);
                uint32_t key[mz::kMtN];
                std::memcpy(key, host.key, sizeof(key));
                int32_t pos = host.pos;
                uint32_t words = 0;
                moves[kind - 1] = mz::opponent_action(game, kind, board, player, key, &pos, &words);
                drawn[kind - 1] = words;
                host.below(static_cast<uint32_t>(n));
                same = same && words == host.words && pos == host.pos && std::memcmp(key, host.key, sizeof(key)) == 0;
                if (kind == mz::kOpponentExpert) expert_pos = pos;
            }
            std::printf("X %d %u %d %d %d %u\n", moves[0], drawn[0], expert_pos, same ? 1 : 0, moves[1], drawn[1]);
        } else {
            return 2;
        }
        ++rows;
    }
    std::printf("{\"rows\": %ld}\n", rows);
    return 0;
}
