// Readers and writers the feature-file tools share: a feature file in the text_output.txt format extract_features writes ("#features",
// then one line of comma-terminated values per row) and an id file with one integer per line.
#ifndef CAFFE_TOOLS_FEATURE_FILES_HPP_
#define CAFFE_TOOLS_FEATURE_FILES_HPP_
#include <cstdio>
#include <fstream>

#include "caffe/layer.hpp"

namespace caffe {

inline void ReadFeatures(const char* path, vector<float>* v, int* rows, int* dim) {
  std::ifstream f(path);
  CHECK(f.good()) << "Failed to open " << path;
  string line;
  *rows = 0; *dim = 0;
  while (std::getline(f, line)) {
    if (line.empty() || line[0] == '#') continue;
    int n = 0;
    const char* p = line.c_str();
    while (*p) {
      char* e = nullptr;
      const float x = strtof(p, &e);
      if (e == p) break;
      v->push_back(x); ++n;
      p = e;
      while (*p == ',' || *p == ' ') ++p;
    }
    if (*rows == 0) *dim = n;
    CHECK_EQ(n, *dim) << "row " << *rows << " of " << path;
    ++*rows;
  }
  CHECK_GT(*rows, 0) << "no feature rows in " << path;
}

inline void ReadIds(const char* path, int rows, Blob<float>* b) {
  std::ifstream f(path);
  CHECK(f.good()) << "Failed to open " << path;
  b->Reshape(rows, 1, 1, 1);
  string line;
  int n = 0;
  while (std::getline(f, line)) {
    if (line.empty() || line[0] == '#') continue;
    CHECK_LT(n, rows) << "more ids than feature rows in " << path;
    const long id = atol(line.c_str());
    CHECK_LT(labs(id), 1l << 24) << "id " << id << " does not survive the float blob the layer reads ids from";
    b->mutable_cpu_data()[n++] = (float)id;
  }
  CHECK_EQ(n, rows) << "ids in " << path;
}

inline void Fill(const vector<float>& v, int rows, int dim, Blob<float>* b) {
  b->Reshape(rows, dim, 1, 1);
  std::copy(v.begin(), v.end(), b->mutable_cpu_data());
}

// rows x dim values in the format ReadFeatures reads, nine significant digits: every fp32 value reads back as itself
inline void WriteFeatures(const char* path, const float* v, int rows, int dim) {
  FILE* f = fopen(path, "w");
  CHECK(f) << "Failed to open " << path;
  fprintf(f, "#features\n");
  for (int r = 0; r < rows; ++r) {
    for (int c = 0; c < dim; ++c) fprintf(f, "%.9g,", (double)v[(size_t)r * dim + c]);
    fprintf(f, "\n");
  }
  CHECK_EQ(fclose(f), 0) << "Failed to write " << path;
}

// one integer per line, the format ReadIds reads
inline void WriteInts(const char* path, const int* v, int rows) {
  FILE* f = fopen(path, "w");
  CHECK(f) << "Failed to open " << path;
  for (int r = 0; r < rows; ++r) fprintf(f, "%d\n", v[r]);
  CHECK_EQ(fclose(f), 0) << "Failed to write " << path;
}

}  // namespace caffe
#endif  // CAFFE_TOOLS_FEATURE_FILES_HPP_
