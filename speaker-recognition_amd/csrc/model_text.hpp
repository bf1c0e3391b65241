// model_text.hpp -- the reference's text model format: GMM::load gmm.cc:664-682 / Gaussian::load :125-150; GMM::dump :655-662 /
// Gaussian::dump :101-123 (default ostream precision = "%g", 6 significant digits).
#pragma once

#include <string>

struct GMM;

namespace sr {

void gmm_parse_text(const std::string &text, GMM &out);
std::string gmm_format_text(const GMM &g);

}  // namespace sr
