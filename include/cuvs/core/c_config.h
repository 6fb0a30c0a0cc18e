/* Optional components of this build — the header the reference generates at configure time
 * (c/CMakeLists.txt:136-152). Both are built: the cuvsMultiGpu* index wrappers (cuvs_amd/csrc/mg.hip) and the HNSW
 * hand-over of a CAGRA graph (CUVS_BUILD_CAGRA_HNSWLIB, <cuvs/neighbors/hnsw.h>: cuvs_amd/csrc/hnsw.hip and hnsw_host.hpp,
 * written here; hnswlib itself is not used). */
#pragma once
#ifndef CUVS_BUILD_MG_ALGOS
#define CUVS_BUILD_MG_ALGOS
#endif
#ifndef CUVS_BUILD_CAGRA_HNSWLIB
#define CUVS_BUILD_CAGRA_HNSWLIB
#endif
