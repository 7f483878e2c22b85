// The fast map <-> circular-buffer index pair of csrc/gridmath.hpp against the general wrap_index forms, on the host alone:
//   map_to_buffer(x, s, n) == wrap_index(x + s, n) and buffer_to_map is its inverse, for every start and every index of
//   n in {1, 2, 63, 64, 65, 130};
//   buffer_lin / map_cell_of the same on a 130 x 70 map, every (s0, s1) from {0, 1, 63, 64, 65, size - 1} per axis, against
//   buffer_index / unwrap_index of a Geom with that start;
//   the line cursor (index_line_cursor, _offset, _step), placed at every t0 that is a multiple of 8 and stepped 8 cells, over
//   every pair of end points of a 13 x 13 box and lines with D = 65535, A in {0, 1, 32767, 65534, 65535}: its offsets equal
//   index_line_cell, its turn flag the difference of index_line_minor at t + 1 and at t.
#include <cstdio>
#include <set>
#include <vector>

#include "../../ros_navigation_amd/csrc/gridmath.hpp"

using namespace rna;

static int fails = 0;
#define CHECK(c)                                                   \
  do {                                                             \
    if (!(c) && fails++ < 10) std::printf("FAILED line %d: %s\n", __LINE__, #c); \
  } while (0)

int main() {
  const int sizes[] = {1, 2, 63, 64, 65, 130};
  long checked = 0;
  for (int n : sizes)
    for (int s = 0; s < n; ++s)
      for (int x = 0; x < n; ++x) {
        const int b = map_to_buffer(x, s, n);
        CHECK(b == wrap_index(x + s, n));
        CHECK(b >= 0 && b < n);
        CHECK(buffer_to_map(b, s, n) == x);
        CHECK(buffer_to_map(x, s, n) == wrap_index(x - s, n));
        ++checked;
      }

  const int rows = 130, cols = 70;
  std::set<int> st0 = {0, 1, 63, 64, 65, rows - 1}, st1 = {0, 1, 63, 64, 65, cols - 1};
  for (int s0 : st0)
    for (int s1 : st1) {
      Geom g;
      set_geometry(g, rows * 0.05, cols * 0.05, 0.05, 0.0, 0.0);
      CHECK(g.size[0] == rows && g.size[1] == cols);
      g.start[0] = s0;
      g.start[1] = s1;
      std::vector<char> seen((size_t)rows * cols, 0);
      for (int j = 0; j < cols; ++j)
        for (int i = 0; i < rows; ++i) {
          const int u[2] = {i, j};
          int b[2], back[2];
          buffer_index(g, u, b);
          const size_t lin = buffer_lin(i, j, rows, cols, s0, s1);
          CHECK(buffer_lin<int>(i, j, rows, cols, s0, s1) == (int)lin && buffer_lin<unsigned>(i, j, rows, cols, s0, s1) == (unsigned)lin);
          CHECK(lin == (size_t)b[1] * rows + b[0]);
          CHECK(lin < seen.size() && !seen[lin]);
          if (lin < seen.size()) seen[lin] = 1;
          unwrap_index(g, b, back);
          CHECK(back[0] == i && back[1] == j);
          int mi, mj;
          map_cell_of(lin, rows, cols, s0, s1, mi, mj);   // a 64-bit index
          CHECK(mi == i && mj == j);
          map_cell_of((int)lin, rows, cols, s0, s1, mi, mj);
          CHECK(mi == i && mj == j);
          map_cell_of((unsigned)lin, rows, cols, s0, s1, mi, mj);
          CHECK(mi == i && mj == j);
          ++checked;
        }
    }
  // the line cursor: every pair of end points of a 13 x 13 box, and lines with D = 65535
  std::vector<IndexLine> lines;
  for (int a = 0; a < 169; ++a)
    for (int b = 0; b < 169; ++b) {
      const int s[2] = {a % 13, a / 13}, e[2] = {b % 13, b / 13};
      lines.push_back(index_line(s, e));
    }
  for (int A : {0, 1, 32767, 65534, 65535})
    for (int k = 0; k < 4; ++k) {   // either major axis, either direction
      const int s[2] = {7, -3}, d[2] = {(k & 1) ? A : 65535, (k & 1) ? 65535 : A};
      const int e[2] = {(k & 2) ? s[0] - d[0] : s[0] + d[0], (k & 2) ? s[1] + d[1] : s[1] - d[1]};
      lines.push_back(index_line(s, e));
      CHECK(lines.back().D == 65535 && lines.back().A == A);
    }
  for (const IndexLine& ln : lines) {
    if (ln.D == 0) continue;   // (a single cell: nothing to walk)
    for (int t0 = 0; t0 <= ln.D; t0 += 8) {
      LineCursor cur = index_line_cursor(ln, t0);
      for (int t = t0; t < t0 + 8 && t <= ln.D; ++t) {
        int d[2], c[2];
        index_line_cursor_offset(ln, cur, d);
        index_line_cell(ln, t, c);
        CHECK(cur.t == t && ln.s[0] + d[0] == c[0] && ln.s[1] + d[1] == c[1]);
        const bool turn = index_line_cursor_step(ln, cur);
        if (t < ln.D) CHECK((int)turn == index_line_minor(ln, t + 1) - index_line_minor(ln, t));
        ++checked;
      }
    }
  }

  if (fails) {
    std::printf("gridmath index: %d checks FAILED\n", fails);
    return 1;
  }
  std::printf("gridmath index ok (%ld cases)\n", checked);
  return 0;
}
