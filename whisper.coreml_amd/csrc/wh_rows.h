// The row table of a first pass (a decode's prompt pass, wh_prefill_logits, an alignment
// pass): every token of every window is one decoder row in beam slot 0 at its position in the
// window.  No HIP in it: tools/rows_host_check.cpp runs it under the host sanitizers.
#pragma once
#include <vector>

namespace wh {

struct RowPlan {
  // per row: token, position in its window, the self-KV window it writes, its beam slot (0)
  std::vector<int> row_tok, row_pos, row_win, row_slot;
  // per window: first row, row count, the encoder slot its cross-attention reads
  std::vector<int> win_row0, win_nrows, win_slot;
  int R = 0;  // rows
  int nw() const { return (int)win_row0.size(); }
  // `win` goes into row_win: the decode's window index for its prompt pass, the encoder slot
  // for the first passes that run outside a decode batch
  void add(int win, int slot, const int* tokens, int n) {
    win_row0.push_back(R);
    win_nrows.push_back(n);
    win_slot.push_back(slot);
    for (int p = 0; p < n; ++p) {
      row_tok.push_back(tokens[p]);
      row_pos.push_back(p);
      row_win.push_back(win);
      row_slot.push_back(0);
    }
    R += n;
  }
};

}  // namespace wh
