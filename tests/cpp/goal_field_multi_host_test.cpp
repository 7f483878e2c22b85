// GPU test of the C++ layer of the goal field with many goals (ros_navigation_amd/host/move_control_amd.hpp): the
// multi-goal GridGoalField constructor, ownerOf, costToGoal, makePlan and assignFrontiers against the values in the case file
// argv[1], which tests/test_gpu_goal_field_multi.py writes from answers it has compared with its oracle:
//   rows cols / rows * cols master values (buffer order of an unmoved map, "nan" = unknown) / n goals / n x (x y seed) /
//   n samples / n x (x y owner cost plan_length; cost -1 = no plan) / n frontiers / their owners in frontiers()'s order
#include <cmath>
#include <cstdio>
#include <vector>

#include "move_control_amd.hpp"

using namespace grid_map;
using namespace move_control;

#define CHECK(c) do { if (!(c)) { std::printf("FAILED line %d: %s\n", __LINE__, #c); return 1; } } while (0)

int main(int argc, char** argv) {
  CHECK(argc == 2);
  FILE* f = std::fopen(argv[1], "r");
  CHECK(f);
  int rows = 0, cols = 0, n = 0;
  CHECK(std::fscanf(f, "%d %d", &rows, &cols) == 2 && rows > 0 && cols > 0);
  std::vector<float> m((size_t)rows * cols);
  for (size_t k = 0; k < m.size(); ++k) CHECK(std::fscanf(f, "%f", &m[k]) == 1);
  GridMap map;
  map.setGeometry(Length(rows * 0.05, cols * 0.05), 0.05);
  CHECK(map.getSize()[0] == rows && map.getSize()[1] == cols);
  map.set("master", m);

  CHECK(std::fscanf(f, "%d", &n) == 1 && n >= 2);
  std::vector<Position> goals;
  std::vector<int32_t> seed;
  for (int k = 0; k < n; ++k) {
    double x, y;
    int s;
    CHECK(std::fscanf(f, "%lf %lf %d", &x, &y, &s) == 3);
    goals.push_back(Position(x, y));
    seed.push_back(s);
  }
  GridGoalField field(map, goals, seed, true);
  CHECK(field.info().status == 0 && field.info().reached > 0 && !field.stale());
  rna_goal_field_sources_info src;
  CHECK(rna_goal_field_sources_info_get(map.engine(), &src) == RNA_OK && src.sources == n && src.owners == 1);

  CHECK(std::fscanf(f, "%d", &n) == 1 && n > 0);
  int plans = 0;
  for (int k = 0; k < n; ++k) {
    double x, y;
    int owner, cost, len;
    CHECK(std::fscanf(f, "%lf %lf %d %d %d", &x, &y, &owner, &cost, &len) == 5);
    Position p(x, y);
    CHECK(field.ownerOf(p) == owner);
    std::vector<Position> path;
    int32_t c = -1;
    if (cost < 0) {
      CHECK(!field.makePlan(p, path) && !field.costToGoal(p, c));
      continue;
    }
    CHECK(owner >= 0 && field.costToGoal(p, c) && c == cost);
    CHECK(field.makePlan(p, path) && (int)path.size() == len);
    const Position& last = path.back();
    CHECK(std::fabs(last[0] - goals[(size_t)owner][0]) < 1e-9 && std::fabs(last[1] - goals[(size_t)owner][1]) < 1e-9);
    ++plans;
  }
  CHECK(plans >= n / 4);
  Position outside(1000.0, 1000.0);
  CHECK(field.ownerOf(outside) == -1);

  std::vector<Frontier> ranked;
  CHECK(field.frontiers(2, ranked));
  CHECK(std::fscanf(f, "%d", &n) == 1 && n == (int)ranked.size() && n > 0);
  const std::vector<int> owners = field.assignFrontiers(ranked);
  CHECK((int)owners.size() == n);
  for (int k = 0; k < n; ++k) {
    int want;
    CHECK(std::fscanf(f, "%d", &want) == 1 && owners[(size_t)k] == want);
    Position p;
    CHECK(map.getPosition(ranked[(size_t)k].nearest, p) && field.ownerOf(p) == want);
  }
  std::fclose(f);

  // the same goals without seeds and without owners: ownerOf is refused, plans still end at a goal; rebuild() keeps the goals
  GridGoalField plain(map, goals);
  CHECK(plain.info().status == 0 && plain.rebuild());
  bool threw = false;
  try { (void)plain.ownerOf(goals[0]); } catch (const std::exception&) { threw = true; }
  CHECK(threw);
  std::vector<Position> path;
  CHECK(plain.makePlan(goals[1], path) && path.size() == 1);
  // a goal outside the map
  std::vector<Position> bad(goals);
  bad.push_back(outside);
  threw = false;
  try { GridGoalField nope(map, bad); } catch (const std::exception&) { threw = true; }
  CHECK(threw);
  std::printf("goal field multi host OK\n");
  return 0;
}
