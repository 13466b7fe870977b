// cvec.h — control-vector GGUF files (what llama-cvector-generator writes and --control-vector reads).  Host arithmetic only.
//
// The file: tensors named direction.N, N >= 1, F32, one dimension, all of one length n_embd; every other tensor and every key is ignored.  Loading follows
// upstream's common_control_vector_load as remembered (unpinned): each file's tensors are accumulated as scale * tensor into layer N's slot,
// several files are summed, and the result holds layers 1 .. the highest layer named, back to back (layer N at n_embd * (N - 1)); a layer no file names is zero.
#pragma once

#include <string>
#include <vector>

namespace mi355 {

struct ControlVectorFile { std::string path; float scale = 1.0f; };

// False with err set (it names the file and the tensor) for: a file that does not open, a tensor direction.0 or direction.<not a number>, a direction tensor
// that is not F32 or not one-dimensional, direction tensors of different lengths within a file or between files, a file without any direction tensor, an
// empty list.
bool control_vector_load(const std::vector<ControlVectorFile> &files, std::vector<float> &data, int &n_embd, std::string &err);

}  // namespace mi355
