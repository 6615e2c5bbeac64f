"""The two names the hooks read: where data sets live (ends with a separator) and which of them have a versioned file name."""
import os

PROJ_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', '')
DATA_VERSION_DICT = {'tgbl-wiki': 2, 'tgbl-review': 2, 'tgbl-coin': 2, 'tgbl-flight': 2, 'tgbl-comment': 1}
