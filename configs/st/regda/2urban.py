"""st.regda.2urban: LoveDA Rural -> Urban (the names of the reference's configs/st/regda/2urban.py)."""
from configs.st.regda._surface import install

install(globals(), 'urban')
