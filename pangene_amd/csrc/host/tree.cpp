// tree.cpp -- the commands over the pairwise fixed-point distances of the assemblies and their tree: ONE translation unit, one header per command with
// its host loops, its run function, its text output and its extern "C" entries, included in this order (a later one uses what an
// earlier one defines).
//   pan_tree.hpp       the fixed-point distances and the entry helpers all four share; the joins, the bootstrap, pangene tree
//   pan_cluster.hpp    k-medoids, pangene cluster
//   pan_permanova.hpp  pangene permanova
//   pan_mantel.hpp     pangene mantel
//   pan_gainloss.hpp   pangene gainloss (with pan_treeprog.hpp: the records as a tree and as the backend's program, shared with trait.cpp)
//   pan_rates.hpp      pangene rates (the program, the item counts and the limits are pan_gainloss.hpp's; floating point)
//   pan_coevo.hpp      pangene coevo (the reconstruction and the program are pan_gainloss.hpp's)
//   pan_phylosig.hpp   pangene phylosig (the observed costs and the way up are pan_gainloss.hpp's)
//   pan_pcoa.hpp       pangene pcoa (floating point: the exact trace uses pan_permanova.hpp's ratio)
//   pan_glm.hpp        pangene glm (the axes are pan_pcoa.hpp's pcoa_core, the trait files trait.cpp's readers)
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <unordered_map>
#include <vector>
#include "pg_internal.hpp"
#include "pan_treeprog.hpp"

using namespace pgx;

#include "pan_tree.hpp"
#include "pan_cluster.hpp"
#include "pan_permanova.hpp"
#include "pan_mantel.hpp"
#include "pan_gainloss.hpp"
#include "pan_rates.hpp"
#include "pan_coevo.hpp"
#include "pan_phylosig.hpp"
#include "pan_pcoa.hpp"
#include "pan_glm.hpp"
